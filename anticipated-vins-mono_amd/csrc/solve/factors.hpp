// solve/factors.hpp - the factors as the reference states them, one thread each: proj_eval, imu_raw, imu_col, prior_block_dx
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

struct Frames {
  const double* R;  // [11][9]
  const double* A;  // [11][9]  ric^T * R_f^T
};

// ---- projection factor (projection_factor.cpp:21-121) -----------------------------------
// out: r[2], Ji[12] (2x6), Jj[12], Je[2]; returns 1/2 rho(|r|^2) ; robustified with CauchyLoss.
template <bool WANT_J>
AVM_DEV double proj_eval(const double* x, Frames fr, const double* ric, const double* tic, double pix, double piy, double pjx,
                         double pjy, double lam, int fa, int fb, double sqi, double cauchy_a, bool apply_loss, double* r,
                         double* Ji, double* Jj, double* Je, double* Jex = nullptr, double* Jtd = nullptr, double vix = 0.0,
                         double viy = 0.0, double vjx = 0.0, double vjy = 0.0) {
  const double* Ra = fr.R + fa * 9;
  const double* Rb = fr.R + fb * 9;
  const v3 Pa = mk3(x[fa * 7], x[fa * 7 + 1], x[fa * 7 + 2]);
  const v3 Pb = mk3(x[fb * 7], x[fb * 7 + 1], x[fb * 7 + 2]);
  const v3 t = mk3(tic[0], tic[1], tic[2]);
  const double il = fast_rcp(lam);
  const v3 pci = mk3(pix * il, piy * il, il);
  const v3 pimu_i = Rmul(ric, pci) + t;
  const v3 pw = Rmul(Ra, pimu_i) + Pa;
  const v3 pimu_j = RTmul(Rb, pw - Pb);
  const v3 pcj = RTmul(ric, pimu_j - t);
  const double dep = pcj.z;
  const double id = fast_rcp(dep);  // one reciprocal per quantity: the quotients below are products with it
  double r0 = sqi * (pcj.x * id - pjx);
  double r1 = sqi * (pcj.y * id - pjy);
  const double sn = r0 * r0 + r1 * r1;
  // ceres::CauchyLoss + Corrector: rho'' < 0 => residual and Jacobian scale by sqrt(rho')
  const double b = cauchy_a * cauchy_a, c = fast_rcp(b);
  const double sum = 1.0 + sn * c;
  const double rho0 = b * log(sum);
  // sqrt(max(DBL_MIN, 1 / sum)), Corrector's sqrt(rho'): 1.4916681462400413e-154 = sqrt(DBL_MIN)
  const double srho = apply_loss ? fmax(fast_rsqrt(sum), 1.4916681462400413e-154) : 1.0;
  r[0] = srho * r0;
  r[1] = srho * r1;
  if (WANT_J) {
    const double* Ab = fr.A + fb * 9;
    const double id2 = id * id;
    // reduce = sqrt_info [1/z 0 -x/z^2; 0 1/z -y/z^2], with the loss scaling folded in: two terms per entry
    const double rd = srho * sqi * id, rx = -(srho * sqi) * (pcj.x * id2), ry = -(srho * sqi) * (pcj.y * id2);
    const double red[6] = {sqi * id, 0.0, sqi * (-pcj.x * id2), 0.0, sqi * id, sqi * (-pcj.y * id2)};
    double M[6], MR[6], N[6];
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      M[cc] = rd * Ab[cc] + rx * Ab[6 + cc];
      M[3 + cc] = rd * Ab[3 + cc] + ry * Ab[6 + cc];
      N[cc] = rd * ric[cc * 3] + rx * ric[cc * 3 + 2];
      N[3 + cc] = rd * ric[cc * 3 + 1] + ry * ric[cc * 3 + 2];
    }
#pragma unroll
    for (int rr = 0; rr < 2; rr++)
#pragma unroll
      for (int cc = 0; cc < 3; cc++) MR[rr * 3 + cc] = M[rr * 3] * Ra[cc] + M[rr * 3 + 1] * Ra[3 + cc] + M[rr * 3 + 2] * Ra[6 + cc];
    const v3 u = Rmul(ric, mk3(pix, piy, 1.0));  // ric * pts_i
    const double il2 = -(il * il);
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
      const v3 m = mk3(M[rr * 3], M[rr * 3 + 1], M[rr * 3 + 2]);
      const v3 mr = mk3(MR[rr * 3], MR[rr * 3 + 1], MR[rr * 3 + 2]);
      const v3 n = mk3(N[rr * 3], N[rr * 3 + 1], N[rr * 3 + 2]);
      const v3 ci = cross(pimu_i, mr);  // mr * (-skew(pts_imu_i))
      const v3 cj = cross(n, pimu_j);   // n * skew(pts_imu_j)
      Ji[rr * 6 + 0] = m.x, Ji[rr * 6 + 1] = m.y, Ji[rr * 6 + 2] = m.z;
      Ji[rr * 6 + 3] = ci.x, Ji[rr * 6 + 4] = ci.y, Ji[rr * 6 + 5] = ci.z;
      Jj[rr * 6 + 0] = -m.x, Jj[rr * 6 + 1] = -m.y, Jj[rr * 6 + 2] = -m.z;
      Jj[rr * 6 + 3] = cj.x, Jj[rr * 6 + 4] = cj.y, Jj[rr * 6 + 5] = cj.z;
      Je[rr] = dot(mr, u) * il2;
      // ProjectionTdFactor (projection_td_factor.cpp:131-136): d r / d td = reduce ric^T Rj^T Ri ric velocity_i (-1 / lambda) +
      // sqrt_info velocity_j; (pix, piy) / (pjx, pjy) are the td-shifted observations then (the caller shifts them)
      if (Jtd) Jtd[rr] = dot(mr, Rmul(ric, mk3(vix, viy, 0.0))) * -il + (srho * sqi) * (rr == 0 ? vjx : vjy);
      if (Jex) {
        // jaco_ex (projection_factor.cpp:97-107): left = ric^T (Rj^T Ri - I); right = -tmp_r [pc_i]x + [tmp_r pc_i]x + [q]x,
        // and tmp_r pc_i + q is the point in camera j, so the two skew terms collapse to [pc_j]x
        const v3 mrr = mk3(mr.x * ric[0] + mr.y * ric[3] + mr.z * ric[6], mr.x * ric[1] + mr.y * ric[4] + mr.z * ric[7],
                           mr.x * ric[2] + mr.y * ric[5] + mr.z * ric[8]);  // (reduce ric^T Rj^T Ri ric) row
        const v3 rho = mk3(srho * red[rr * 3], srho * red[rr * 3 + 1], srho * red[rr * 3 + 2]);
        const v3 ex_r = cross(pci, mrr) + cross(rho, pcj);
        Jex[rr * 6 + 0] = mr.x - n.x, Jex[rr * 6 + 1] = mr.y - n.y, Jex[rr * 6 + 2] = mr.z - n.z;
        Jex[rr * 6 + 3] = ex_r.x, Jex[rr * 6 + 4] = ex_r.y, Jex[rr * 6 + 5] = ex_r.z;
      }
    }
  }
  return 0.5 * rho0;
}

// ---- IMU factor, raw part before sqrt_info (imu_factor.h:60-175, integration_base.h:160-186).
// One thread evaluates factor i; writes raw residual (15) and, if WANT_J, the raw 15x30
// Jacobian (pose_i 6 | sb_i 9 | pose_j 6 | sb_j 9) into stage[0..465) laid out [15][31]
// (col 0 = residual).  stage must be zeroed beforehand.
template <bool WANT_J>
AVM_DEV void imu_raw(const double* x, const double* Rfr, const avm_options& o, const double* delta, const double* pj /*15x15*/,
                     double sum_dt, const double* lba, const double* lbg, int i, double* stage) {
  const int j = i + 1;
  const v3 Pi = mk3(x[i * 7], x[i * 7 + 1], x[i * 7 + 2]), Pj = mk3(x[j * 7], x[j * 7 + 1], x[j * 7 + 2]);
  const quat Qi{x[i * 7 + 6], x[i * 7 + 3], x[i * 7 + 4], x[i * 7 + 5]}, Qj{x[j * 7 + 6], x[j * 7 + 3], x[j * 7 + 4], x[j * 7 + 5]};
  const double* si = x + XSB + i * 9;
  const double* sj = x + XSB + j * 9;
  const v3 Vi = mk3(si[0], si[1], si[2]), Bai = mk3(si[3], si[4], si[5]), Bgi = mk3(si[6], si[7], si[8]);
  const v3 Vj = mk3(sj[0], sj[1], sj[2]), Baj = mk3(sj[3], sj[4], sj[5]), Bgj = mk3(sj[6], sj[7], sj[8]);
  const v3 G = mk3(o.g[0], o.g[1], o.g[2]);
  const v3 dP = mk3(delta[0], delta[1], delta[2]), dV = mk3(delta[7], delta[8], delta[9]);
  const quat dQ{delta[6], delta[3], delta[4], delta[5]};
  auto blk = [&](int r0, int c0, double* M) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) M[a * 3 + b] = pj[(r0 + a) * 15 + c0 + b];
  };
  double dp_dba[9], dp_dbg[9], dq_dbg[9], dv_dba[9], dv_dbg[9];
  blk(0, 9, dp_dba), blk(0, 12, dp_dbg), blk(3, 12, dq_dbg), blk(6, 9, dv_dba), blk(6, 12, dv_dbg);
  const v3 dba = Bai - mk3(lba[0], lba[1], lba[2]), dbg = Bgi - mk3(lbg[0], lbg[1], lbg[2]);
  const quat cdq = qmul(dQ, deltaQ(Rmul(dq_dbg, dbg)));
  const v3 cdv = dV + Rmul(dv_dba, dba) + Rmul(dv_dbg, dbg);
  const v3 cdp = dP + Rmul(dp_dba, dba) + Rmul(dp_dbg, dbg);
  const quat Qi_inv = qinv(Qi);
  const v3 tp = qrot(Qi_inv, (0.5 * sum_dt * sum_dt) * G + Pj - Pi - sum_dt * Vi);
  const v3 tv = qrot(Qi_inv, sum_dt * G + Vj - Vi);
  const v3 rp = tp - cdp;
  const quat qe = qmul(qinv(cdq), qmul(Qi_inv, Qj));
  const v3 rr = mk3(2.0 * qe.x, 2.0 * qe.y, 2.0 * qe.z);
  const v3 rv = tv - cdv;
  const v3 rba = Baj - Bai, rbg = Bgj - Bgi;
  for (int k = 0; k < 3; k++) {
    stage[(0 + k) * 31] = get(rp, k);
    stage[(3 + k) * 31] = get(rr, k);
    stage[(6 + k) * 31] = get(rv, k);
    stage[(9 + k) * 31] = get(rba, k);
    stage[(12 + k) * 31] = get(rbg, k);
  }
  if (WANT_J) {
    const double* Ri = Rfr + i * 9;  // R_i ; R_i^T = (Qi.inverse()).toRotationMatrix() for unit Qi
    auto put = [&](int r0, int c0, const double* M, double sgn) {
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) stage[(r0 + a) * 31 + 1 + c0 + b] = sgn * M[a * 3 + b];
    };
    double RiT[9];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) RiT[a * 3 + b] = Ri[b * 3 + a];
    double M[9], M2[9];
    // pose_i (cols 0..5)
    put(0, 0, RiT, -1.0);
    skew9(tp, M);
    put(0, 3, M, 1.0);
    qleft_qright_br(qmul(qinv(Qj), Qi), cdq, M);
    put(3, 3, M, -1.0);
    skew9(tv, M);
    put(6, 3, M, 1.0);
    // speedbias_i (cols 6..14): V 6.., BA 9.., BG 12..
    for (int a = 0; a < 9; a++) M[a] = RiT[a] * sum_dt;
    put(0, 6, M, -1.0);
    put(0, 9, dp_dba, -1.0);
    put(0, 12, dp_dbg, -1.0);
    qleft_br(qmul(qmul(qinv(Qj), Qi), dQ), M);
    mat3mul(M, dq_dbg, M2);
    put(3, 12, M2, -1.0);
    put(6, 6, RiT, -1.0);
    put(6, 9, dv_dba, -1.0);
    put(6, 12, dv_dbg, -1.0);
    for (int a = 0; a < 3; a++) {
      stage[(9 + a) * 31 + 1 + 9 + a] = -1.0;
      stage[(12 + a) * 31 + 1 + 12 + a] = -1.0;
    }
    // pose_j (cols 15..20)
    put(0, 15, RiT, 1.0);
    qleft_br(qmul(qmul(qinv(cdq), Qi_inv), Qj), M);
    put(3, 18, M, 1.0);
    // speedbias_j (cols 21..29)
    put(6, 21, RiT, 1.0);
    for (int a = 0; a < 3; a++) {
      stage[(9 + a) * 31 + 1 + 24 + a] = 1.0;
      stage[(12 + a) * 31 + 1 + 27 + a] = 1.0;
    }
  }
}

// state column of IMU-factor-local column c (0..29) for factor i
AVM_DEV int imu_col(int i, int c) {
  if (c < 6) return 6 * i + c;
  if (c < 15) return SB0 + 9 * i + (c - 6);
  if (c < 21) return 6 * (i + 1) + (c - 15);
  return SB0 + 9 * (i + 1) + (c - 21);
}

// MarginalizationFactor dx of one kept block (marginalization_factor.cpp:346-363)
AVM_DEV void prior_block_dx(int kind, const double* xb, const double* x0, double* dx) {
  if (kind == AVM_BLK_SPEEDBIAS) {
    for (int k = 0; k < 9; k++) dx[k] = xb[k] - x0[k];
  } else if (kind == AVM_BLK_TD) {
    dx[0] = xb[0] - x0[0];
  } else {
    for (int k = 0; k < 3; k++) dx[k] = xb[k] - x0[k];
    const quat q0{x0[6], x0[3], x0[4], x0[5]}, q{xb[6], xb[3], xb[4], xb[5]};
    const quat d = qmul(qinv(q0), q);
    const double sg = (d.w >= 0) ? 2.0 : -2.0;
    dx[3] = sg * d.x, dx[4] = sg * d.y, dx[5] = sg * d.z;
  }
}
