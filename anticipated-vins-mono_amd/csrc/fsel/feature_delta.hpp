// fsel/feature_delta.hpp - Delta_ell of one feature: feature_front, feature_front4, feature_pair, feature_delta
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

template <bool WAVE>
AVM_DEV double nn_depth(const avm_fsel_batch& b, const double* kd, int p, double fx_, double fy_) {
  return kd_depth<WAVE ? 64 : 1>(b, kd, p, fx_, fy_);
}

// Delta_ell position blocks of one feature (calcInfoFromFeatures), written as dense T x T.
// cam[h] (h = 1..H): t_WC (3), R of q_WC^-1 (9), R of (q_WC * q_IC)^-1 (9)  => 21 doubles per h
// front part: per-frame blocks C_h (Ch, 6 per h), W = (sum C_h)^-1 (Wm); false if the feature is seen in no future frame
// WAVE: called by all 64 lanes of a wavefront for the same feature - the leaves of the nearest-neighbour search are split over the lanes
template <bool WAVE>
AVM_DEV bool feature_front(const avm_fsel_batch& b, const double* kd, int p, const double* cam, double fx_, double fy_, int H, double* Ch /*13*6*/, double* Wm /*9*/) {
  const double dep = nn_depth<WAVE>(b, kd, p, fx_, fy_);
  const double nrm = sqrt(fx_ * fx_ + fy_ * fy_ + 1.0);
  const v3 fn = mk3(fx_ / nrm, fy_ / nrm, 1.0 / nrm);  // feature.normalized()
  const v3 feat = dep * fn;
  // pell = t_WC_k1 + q_WC_k1 * feature  (R of q_WC^-1 is the transpose of R(q_WC) for unit quaternions; the
  // oracle rotates with the quaternion itself; cam[1] block stores R(q_WC) too at +21*H.. see setup)
  const double* c1 = cam + 1 * 30;
  const v3 pell = mk3(c1[0], c1[1], c1[2]) + Rmul(c1 + 21, feat);
  int numVisible = 1;
  for (int i = 0; i < H * 6; i++) Ch[i] = 0.0;  // symmetric 3x3 per h: xx xy xz yy yz zz
  double E[6] = {0, 0, 0, 0, 0, 0};
  auto addC = [&](int hidx, v3 u, const double* Rinv2) {
    // Bh = skew(u) * Rinv2 ; C = Bh^T Bh
    double S[9], Bm[9];
    skew9(u, S);
    mat3mul(S, Rinv2, Bm);
    double* C = Ch + hidx * 6;
    C[0] = Bm[0] * Bm[0] + Bm[3] * Bm[3] + Bm[6] * Bm[6];
    C[1] = Bm[0] * Bm[1] + Bm[3] * Bm[4] + Bm[6] * Bm[7];
    C[2] = Bm[0] * Bm[2] + Bm[3] * Bm[5] + Bm[6] * Bm[8];
    C[3] = Bm[1] * Bm[1] + Bm[4] * Bm[4] + Bm[7] * Bm[7];
    C[4] = Bm[1] * Bm[2] + Bm[4] * Bm[5] + Bm[7] * Bm[8];
    C[5] = Bm[2] * Bm[2] + Bm[5] * Bm[5] + Bm[8] * Bm[8];
    for (int k = 0; k < 6; k++) E[k] += C[k];
  };
  for (int h = 2; h <= H; ++h) {
    const double* ch = cam + h * 30;
    const v3 tw = mk3(ch[0], ch[1], ch[2]);
    v3 ue = Rmul(ch + 3, pell - tw);  // q_WC_h^-1 * (pell - t_WC_h)
    const double n = sqrt(dot(ue, ue));
    ue = mk3(ue.x / n, ue.y / n, ue.z / n);
    // PinholeCamera::spaceToPlane with radial-tangential distortion
    const double xu = ue.x / ue.z, yu = ue.y / ue.z;
    const double mx2 = xu * xu, my2 = yu * yu, mxy = xu * yu, rho2 = mx2 + my2;
    const double rad = b.k1 * rho2 + b.k2 * rho2 * rho2;
    const double dxx = xu * rad + 2.0 * b.p1 * mxy + b.p2 * (rho2 + 2.0 * mx2);
    const double dyy = yu * rad + 2.0 * b.p2 * mxy + b.p1 * (rho2 + 2.0 * my2);
    const double pu = b.fx * (xu + dxx) + b.cx, pv = b.fy * (yu + dyy) + b.cy;
    const int iu = (int)round(pu), ivv = (int)round(pv);  // std::round: half away from zero
    // a NaN pixel is outside the image: the reference's double -> int conversion yields INT_MIN for it (x86 cvttsd2si),
    // v_cvt_i32_f64 would yield 0
    if (!(pu == pu && pv == pv && (0 <= iu && iu < b.image_width) && (0 <= ivv && ivv < b.image_height))) continue;
    addC(h - 1, ue, ch + 12);
    ++numVisible;
  }
  if (numVisible == 1) return false;
  addC(0, fn, c1 + 12);
  // W = EtE^-1 (cofactors / det)
  const double a00 = E[0], a01 = E[1], a02 = E[2], a11 = E[3], a12 = E[4], a22 = E[5];
  {
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c10 = a12 * a02 - a01 * a22, c11 = a00 * a22 - a02 * a02, c12 = a02 * a01 - a00 * a12;
    const double c20 = a01 * a12 - a11 * a02, c21 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = a00 * c00 + a01 * c10 + a02 * c20;
    const double id = 1.0 / det;
    Wm[0] = id * c00, Wm[1] = id * c01, Wm[2] = id * c02, Wm[3] = id * c10, Wm[4] = id * c11, Wm[5] = id * c12, Wm[6] = id * c20,
    Wm[7] = id * c21, Wm[8] = id * c22;
  }
  return true;
}

// feature_front for FOUR candidates per wavefront at once (round 4): candidate u on the 16-lane row u, horizon frame h = 1 + (lane & 15) on
// its lanes.  The frames of a candidate are independent until E = sum_h C_h: every lane does ONE frame's projection, visibility test and C_h
// (the one-candidate form did the H of them one after the other on 64 identical lanes), the nearest cloud point is searched by the row's 16
// lanes (kd_depth<16>), C_h goes to the row's LDS record wlu[6 h' + k] (h' = h - 1; zeros for a frame that does not see the feature, as before), and E is
// summed from there IN THE SAME ORDER as feature_front sums it (frames 2 .. H, then frame 1) - the Deltas are bit-identical to the
// one-candidate form's.  Returns (to every lane of the row) whether the candidate is visible from a second frame; W at wlu[6 H ..].
AVM_DEV bool feature_front4(const avm_fsel_batch& b, const double* kd, int p, const double* cam, int k, bool have, int H, double* wlu) {
  const int lane = threadIdx.x & 63, hl = lane & 15, h = hl + 1;
  const double* xy = b.cand_xy + ((size_t)p * b.max_cand + (have ? k : 0)) * 2;
  const double fx_ = xy[0], fy_ = xy[1];
  // findNNDepth by the row's 16 lanes (kd_depth<16>: the reference's kd-tree search, a leaf's points across the lanes)
  const double dep = kd_depth<16>(b, kd, p, fx_, fy_);
  const double nrm = sqrt(fx_ * fx_ + fy_ * fy_ + 1.0);
  const v3 fn = mk3(fx_ / nrm, fy_ / nrm, 1.0 / nrm);
  const v3 feat = dep * fn;
  const double* c1 = cam + 1 * 30;
  const v3 pell = mk3(c1[0], c1[1], c1[2]) + Rmul(c1 + 21, feat);
  double C[6] = {0, 0, 0, 0, 0, 0};
  bool vis = false;
  if (h <= H) {
    const double* ch = cam + h * 30;
    v3 ue = fn;
    if (h >= 2) {
      const v3 tw = mk3(ch[0], ch[1], ch[2]);
      ue = Rmul(ch + 3, pell - tw);
      const double n = sqrt(dot(ue, ue));
      ue = mk3(ue.x / n, ue.y / n, ue.z / n);
      const double xu = ue.x / ue.z, yu = ue.y / ue.z;
      const double mx2 = xu * xu, my2 = yu * yu, mxy = xu * yu, rho2 = mx2 + my2;
      const double rad = b.k1 * rho2 + b.k2 * rho2 * rho2;
      const double dxx = xu * rad + 2.0 * b.p1 * mxy + b.p2 * (rho2 + 2.0 * mx2);
      const double dyy = yu * rad + 2.0 * b.p2 * mxy + b.p1 * (rho2 + 2.0 * my2);
      const double pu = b.fx * (xu + dxx) + b.cx, pv = b.fy * (yu + dyy) + b.cy;
      const int iu = (int)round(pu), ivv = (int)round(pv);
      vis = pu == pu && pv == pv && (0 <= iu && iu < b.image_width) && (0 <= ivv && ivv < b.image_height);
    }
    if (vis || h == 1) {
      double S[9], Bm[9];
      skew9(ue, S);
      mat3mul(S, ch + 12, Bm);
      C[0] = Bm[0] * Bm[0] + Bm[3] * Bm[3] + Bm[6] * Bm[6];
      C[1] = Bm[0] * Bm[1] + Bm[3] * Bm[4] + Bm[6] * Bm[7];
      C[2] = Bm[0] * Bm[2] + Bm[3] * Bm[5] + Bm[6] * Bm[8];
      C[3] = Bm[1] * Bm[1] + Bm[4] * Bm[4] + Bm[7] * Bm[7];
      C[4] = Bm[1] * Bm[2] + Bm[4] * Bm[5] + Bm[7] * Bm[8];
      C[5] = Bm[2] * Bm[2] + Bm[5] * Bm[5] + Bm[8] * Bm[8];
    }
#pragma unroll
    for (int q = 0; q < 6; q++) wlu[6 * (h - 1) + q] = C[q];
  }
  const unsigned long long bal = __ballot(vis);
  const bool ok = have && ((bal >> (lane & 48)) & 0xffffull) != 0;  // numVisible > 1
  wave_lds_sync();
  // E in feature_front's order: frames 2 .. H as the loop met them (an invisible frame adds an exact zero), then frame 1
  double E[6];
#pragma unroll
  for (int q = 0; q < 6; q++) {
    double e = 0.0;
    for (int hh = 2; hh <= H; hh++) e += wlu[6 * (hh - 1) + q];
    E[q] = e + wlu[q];
  }
  const double a00 = E[0], a01 = E[1], a02 = E[2], a11 = E[3], a12 = E[4], a22 = E[5];
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double c10 = a12 * a02 - a01 * a22, c11 = a00 * a22 - a02 * a02, c12 = a02 * a01 - a00 * a12;
  const double c20 = a01 * a12 - a11 * a02, c21 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c10 + a02 * c20;
  const double id = 1.0 / det;
  if (hl == 0) {
    double* Wm = wlu + 6 * H;
    Wm[0] = id * c00, Wm[1] = id * c01, Wm[2] = id * c02, Wm[3] = id * c10, Wm[4] = id * c11, Wm[5] = id * c12, Wm[6] = id * c20,
    Wm[7] = id * c21, Wm[8] = id * c22;
  }
  return ok;
}

// block (i, j), 1 <= j <= i <= H, of Delta_ell = blkdiag(C_h) - [C_i W C_j^T] (and its mirror image), dense T x T
AVM_DEV void feature_pair(const double* Ch, const double* Wm, int i, int j, int T, double* out) {
  auto full = [&](int hidx, double* M) {
    const double* C = Ch + hidx * 6;
    M[0] = C[0], M[1] = C[1], M[2] = C[2], M[3] = C[1], M[4] = C[3], M[5] = C[4], M[6] = C[2], M[7] = C[4], M[8] = C[5];
  };
  double Cj[9], Ci[9], CW[9], D[9];
  full(j - 1, Cj);
  full(i - 1, Ci);
  mat3mul(Ci, Wm, CW);
  // Dij = Ci * W * Cj^T
  for (int a = 0; a < 3; a++)
    for (int c = 0; c < 3; c++) D[a * 3 + c] = CW[a * 3] * Cj[c * 3] + CW[a * 3 + 1] * Cj[c * 3 + 1] + CW[a * 3 + 2] * Cj[c * 3 + 2];
  for (int a = 0; a < 3; a++)
    for (int c = 0; c < 3; c++) {
      const int r = 3 * (i - 1) + a, q = 3 * (j - 1) + c;
      if (i == j) {
        out[r * T + q] = Ci[a * 3 + c] - D[a * 3 + c];
      } else {
        out[r * T + q] = -D[a * 3 + c];
        out[q * T + r] = -D[a * 3 + c];
      }
    }
}

// Delta_ell of one feature by one thread (the used subset; the candidates go one per wavefront, see fsel_setup_kernel)
AVM_DEV bool feature_delta(const avm_fsel_batch& b, const double* kd, int p, const double* cam, double fx_, double fy_, int H, double* out /*T*T*/) {
  double Ch[13 * 6], Wm[9];
  if (!feature_front<false>(b, kd, p, cam, fx_, fy_, H, Ch, Wm)) return false;
  for (int j = 1; j <= H; ++j)
    for (int i = j; i <= H; ++i) feature_pair(Ch, Wm, i, j, 3 * H, out);
  return true;
}
