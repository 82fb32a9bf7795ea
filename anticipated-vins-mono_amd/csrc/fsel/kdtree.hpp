// fsel/kdtree.hpp - findNNDepth: nanoflann's kd-tree, built by fsel_kdtree_kernel and searched without a stack by kd_depth
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

// ---- findNNDepth (feature_selector.cpp:437-459): the reference's kd-tree, bit for bit -------------------------------------------
// The reference asks nanoflann (vendored, vins_estimator/lib/nanoflann/nanoflann.hpp; KDTreeSingleIndexAdaptor<L2_Simple_Adaptor<double>, ., 2>,
// leaf_max_size 10, feature_selector.cpp:424-429) for the 1-NN of the candidate among the window's landmarks and uses that landmark's depth.
// The search is exact, so WHICH point it returns only depends on the tree when several points are at bit-identical distances - and
// then it is the one the traversal meets first (KNNResultSet::addPoint :175-202 replaces on a strictly smaller distance only).  That
// order is part of the reference's behaviour (selected ids are compared bit-exact), so the tree is built here as nanoflann builds it:
//   divideTree :857-907 - a range of <= 10 indices is a leaf; else middleSplit_ :909-958 picks the dimension of largest spread among
//   those whose bounding-box span is within 1e-5 of the largest, cuts at the box's middle clamped to the points' range, planeSplit
//   :969-1005 partitions the index range Hoare-style (< cut | == cut | > cut) and the split position is lim1 / lim2 / count / 2;
//   divlow / divhigh of a node are the children's tightened boxes = max of the left points / min of the right points in the cut dimension;
//   searchLevel :1346-1405 - nearer child first ((val - divlow) + (val - divhigh) < 0), the other one if mindistsq <= worst, a leaf's
//   points in index-array order against the worst distance read at the leaf's entry; computeInitialDistances :1007-1026 from the root box.
// fsel_kdtree_kernel builds it with one wavefront per frame (the partitions as ballot / prefix-count permutations: Hoare's swaps pair
// the i-th misplaced index from the left with the i-th from the right, which is what the sequential loop does), kd_depth walks it
// without a stack: the state of searchLevel's recursion along the current root-to-leaf path is a bit per level (near or far child),
// and (mindistsq, dists[]) are functions of that path, recomputed on the way down - the same additions in the same order.
// Arithmetic that decides comparisons is kept un-contracted (no FMA: the reference's x86 build has none).
// Known-answer tests: tests/test_nanoflann_nn.py (16 928 queries answered by the reference's own header, 4 237 of them exact ties).
struct KdNode {   // 32 bytes
  int a, b;       // inner node: children; leaf: the range [a, b) of the permuted point arrays
  int feat, pad;  // cut dimension (0 / 1); -1: leaf
  double lo, hi;  // divlow, divhigh
};
constexpr int KD_HDR = 8;  // doubles: root box low0 high0 low1 high1 | n_nodes, max_depth (two ints) | -
__host__ __device__ constexpr size_t kd_stride(int max_cloud) { return KD_HDR + (size_t)11 * max_cloud; }  // header | 2 mc nodes (4 doubles each) | xy[mc][2] | depth[mc], in tree order
constexpr int KD_MAXW = 64;  // path words of 64 levels each beyond the first (a tree of n points is at most n - 10 deep)

// minimum / maximum over the wavefront, the result in every lane: four DPP exchange steps inside the 16-lane rows (dpp_d, devmath.hpp: two
// 32-bit moves each), then the four row results through SGPRs - a __shfl_xor ladder is twelve dependent ds_bpermute per double (1.5 K
// cycles; the tree of a 150-point cloud takes ~90 of these reductions).  kd_wave_max is fs_wave_max's ladder, but reads each pair of row
// results right before it compares them; written either way for both users, the compiler schedules one of them differently.
AVM_DEV double kd_wave_min(double v) {
  v = fmin(v, dpp_d<0xB1>(v)), v = fmin(v, dpp_d<0x4E>(v)), v = fmin(v, dpp_d<0x141>(v)), v = fmin(v, dpp_d<0x140>(v));
  return fmin(fmin(readlane_d(v, 0), readlane_d(v, 16)), fmin(readlane_d(v, 32), readlane_d(v, 48)));
}
AVM_DEV double kd_wave_max(double v) {
  v = fmax(v, dpp_d<0xB1>(v)), v = fmax(v, dpp_d<0x4E>(v)), v = fmax(v, dpp_d<0x141>(v)), v = fmax(v, dpp_d<0x140>(v));
  return fmax(fmax(readlane_d(v, 0), readlane_d(v, 16)), fmax(readlane_d(v, 32), readlane_d(v, 48)));
}

// initKDTree (feature_selector.cpp:380-432, the buildIndex part): one wavefront per frame.  LDS: x[mc] y[mc] (doubles), vind[mc], two
// work lists [mc] (ints), a stack of pending ranges.  A node's work depends on its own index range and the box handed down only, so
// the larger child is parked and the smaller one taken first: the stack stays below log2(n) entries whatever the tree's shape.
struct KdPending {
  int l, r, slot, depth;
  double bb[4];
};
constexpr int KD_STACK = 40;
__global__ __launch_bounds__(64) void fsel_kdtree_kernel(FselDev A) {
#pragma clang fp contract(off)
  FS_TABLES_GUARD(A);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const avm_fsel_batch& b = A.b;
  const int p = blockIdx.x, lane = threadIdx.x, mc = b.max_cloud;
  const int n = b.n_cloud ? b.n_cloud[p] : 0;
  if (n <= 0) return;  // (findNNDepth answers 1.0 without a tree)
  double* X = reinterpret_cast<double*>(smem_raw);
  double* Y = X + mc;
  KdPending* stk = reinterpret_cast<KdPending*>(Y + mc);
  int* vi = reinterpret_cast<int*>(stk + KD_STACK);
  int* lml = vi + mc;   // positions of the misplaced indices of the left part, ascending
  int* lmr = lml + mc;  // ... of the right part, ascending
  double* kd = A.kd + (size_t)p * kd_stride(mc);
  KdNode* nodes = reinterpret_cast<KdNode*>(kd + KD_HDR);
  const double* cxy = b.cloud_xy + (size_t)p * mc * 2;
  double lo0 = DBL_MAX, hi0 = -DBL_MAX, lo1 = DBL_MAX, hi1 = -DBL_MAX;
  for (int i = lane; i < n; i += 64) {
    const double x = cxy[2 * i], y = cxy[2 * i + 1];
    X[i] = x, Y[i] = y, vi[i] = i;
    lo0 = fmin(lo0, x), hi0 = fmax(hi0, x), lo1 = fmin(lo1, y), hi1 = fmax(hi1, y);
  }
  lo0 = kd_wave_min(lo0), hi0 = kd_wave_max(hi0), lo1 = kd_wave_min(lo1), hi1 = kd_wave_max(hi1);  // computeBoundingBox
  wave_lds_sync();
  auto coord = [&](int pos, int dim) { return dim == 0 ? X[vi[pos]] : Y[vi[pos]]; };
  // min / max of one coordinate over the index range [l, r)
  auto minmax = [&](int l, int r, int dim, double& mn, double& mx) {
    double a = DBL_MAX, c = -DBL_MAX;
    for (int q = l + lane; q < r; q += 64) {
      const double v = coord(q, dim);
      a = fmin(a, v), c = fmax(c, v);
    }
    mn = kd_wave_min(a), mx = kd_wave_max(c);
  };
  // one pass of planeSplit over [l, l + cnt): indices whose coordinate is < cut (strict) or <= cut to the front; returns how many
  auto partition = [&](int l, int cnt, int dim, double cut, bool strict) {
    int nl = 0;
    for (int base = 0; base < cnt; base += 64) {
      const int q = base + lane;
      const double v = q < cnt ? coord(l + q, dim) : 0.0;
      nl += __popcll(__ballot(q < cnt && (strict ? v < cut : v <= cut)));
    }
    int nml = 0, nmr = 0;
    for (int base = 0; base < cnt; base += 64) {
      const int q = base + lane;
      const double v = q < cnt ? coord(l + q, dim) : 0.0;
      const bool f = q < cnt && (strict ? v < cut : v <= cut);
      const bool ml = q < cnt && !f && q < nl, mr = f && q >= nl;
      const unsigned long long bl = __ballot(ml), br = __ballot(mr), lt = (1ull << lane) - 1ull;
      if (ml) lml[nml + __popcll(bl & lt)] = q;
      if (mr) lmr[nmr + __popcll(br & lt)] = q;
      nml += __popcll(bl), nmr += __popcll(br);
    }
    wave_lds_sync();
    // Hoare's swaps: the i-th misplaced index from the left with the i-th from the right (nml == nmr)
    for (int i = lane; i < nml; i += 64) {
      const int qa = l + lml[i], qb = l + lmr[nml - 1 - i];
      const int t = vi[qa];
      vi[qa] = vi[qb], vi[qb] = t;
    }
    wave_lds_sync();
    return nl;
  };
  int nn = 1, sp = 0, maxdepth = 0;
  int l = 0, r = n, slot = 0, depth = 0;
  double bb[4] = {lo0, hi0, lo1, hi1};
  for (;;) {
    const int cnt = r - l;
    maxdepth = max(maxdepth, depth);
    if (cnt <= 10) {  // a leaf
      if (lane == 0) nodes[slot] = KdNode{l, r, -1, 0, 0.0, 0.0};
      if (sp == 0) break;
      sp--;
      l = stk[sp].l, r = stk[sp].r, slot = stk[sp].slot, depth = stk[sp].depth;
#pragma unroll
      for (int k = 0; k < 4; k++) bb[k] = stk[sp].bb[k];
      continue;
    }
    // middleSplit_
    const double EPS = 0.00001;
    const double span0 = bb[1] - bb[0], span1 = bb[3] - bb[2];
    double max_span = span0;
    if (span1 > max_span) max_span = span1;
    double max_spread = -1.0, mn = 0, mx = 0;
    int cutfeat = 0;
    if (span0 > (1 - EPS) * max_span) {
      double a, c;
      minmax(l, r, 0, a, c);
      const double spread = c - a;
      if (spread > max_spread) cutfeat = 0, max_spread = spread;
      mn = a, mx = c;
    }
    if (span1 > (1 - EPS) * max_span) {
      double a, c;
      minmax(l, r, 1, a, c);
      const double spread = c - a;
      if (spread > max_spread) cutfeat = 1, max_spread = spread, mn = a, mx = c;
    }
    if (max_spread < 0) minmax(l, r, 0, mn, mx);  // (no dimension passed the test: NaN boxes; cutfeat stays 0 like the reference's)
    const double split_val = (bb[2 * cutfeat] + bb[2 * cutfeat + 1]) / 2;
    const double cutval = split_val < mn ? mn : (split_val > mx ? mx : split_val);
    const int lim1 = partition(l, cnt, cutfeat, cutval, true);
    const int lim2 = lim1 + partition(l + lim1, cnt - lim1, cutfeat, cutval, false);
    int idx = lim1 > cnt / 2 ? lim1 : (lim2 < cnt / 2 ? lim2 : cnt / 2);
    idx = min(max(idx, 1), cnt - 1);  // (both children non-empty: holds for every finite cloud, keeps the loop finite for any other)
    double dl, dh, tmp;
    minmax(l, l + idx, cutfeat, tmp, dl);  // divlow: the left child's tightened box, high side
    minmax(l + idx, r, cutfeat, dh, tmp);  // divhigh: the right child's, low side
    const int c1 = nn, c2 = nn + 1;
    nn += 2;
    if (lane == 0) nodes[slot] = KdNode{c1, c2, cutfeat, 0, dl, dh};
    // children: (l, l + idx) with the box cut at high = cutval, (l + idx, r) with low = cutval; the smaller one now, the other parked
    const bool left_now = idx <= cnt - idx;
    if (lane == 0 && sp < KD_STACK) {
      KdPending& e = stk[sp];
      e.l = left_now ? l + idx : l, e.r = left_now ? r : l + idx, e.slot = left_now ? c2 : c1, e.depth = depth + 1;
#pragma unroll
      for (int k = 0; k < 4; k++) e.bb[k] = bb[k];
      e.bb[left_now ? 2 * cutfeat : 2 * cutfeat + 1] = cutval;
    }
    sp++;
    wave_lds_sync();
    if (left_now) r = l + idx, bb[2 * cutfeat + 1] = cutval, slot = c1;
    else l = l + idx, bb[2 * cutfeat] = cutval, slot = c2;
    depth++;
  }
  // header + the points and their depths in tree order (a leaf reads consecutive entries)
  if (lane == 0) {
    kd[0] = lo0, kd[1] = hi0, kd[2] = lo1, kd[3] = hi1;
    int* hi = reinterpret_cast<int*>(kd + 4);
    hi[0] = nn, hi[1] = maxdepth;
  }
  double* pxy = kd + KD_HDR + 8 * (size_t)mc;
  double* pdep = pxy + 2 * (size_t)mc;
  const double* cdep = b.cloud_depth + (size_t)p * mc;
  for (int i = lane; i < n; i += 64) {
    const int o = vi[i];
    pxy[2 * i] = X[o], pxy[2 * i + 1] = Y[o], pdep[i] = cdep[o];
  }
}
// findNeighbors + searchLevel for ONE query by W cooperating lanes (1, 16 or 64 consecutive lanes that enter together with the same
// query): everything is uniform over the group except the leaf scan, where lane i of the group takes the leaf's i-th point.
// Returns findNNDepth's value: the depth of the point the reference's search returns (ret_index stays 0 if nothing is ever closer
// than the initial worst distance, e.g. for a NaN query: then the depth of cloud point 0), 1.0 for an empty cloud.
template <int W>
AVM_DEV double kd_depth(const avm_fsel_batch& b, const double* kdall, int p, double qx, double qy) {
#pragma clang fp contract(off)
  const int n = b.n_cloud ? b.n_cloud[p] : 0;
  if (n <= 0) return 1.0;
  const int mc = b.max_cloud, gl = threadIdx.x & (W - 1);
  const double* kd = kdall + (size_t)p * kd_stride(mc);
  const KdNode* nodes = reinterpret_cast<const KdNode*>(kd + KD_HDR);
  const double* pxy = kd + KD_HDR + 8 * (size_t)mc;
  const double* pdep = pxy + 2 * (size_t)mc;
  // computeInitialDistances
  double di0 = 0.0, di1 = 0.0, dsq = 0.0;
  if (qx < kd[0]) di0 = (qx - kd[0]) * (qx - kd[0]), dsq += di0;
  if (qx > kd[1]) di0 = (qx - kd[1]) * (qx - kd[1]), dsq += di0;
  if (qy < kd[2]) di1 = (qy - kd[2]) * (qy - kd[2]), dsq += di1;
  if (qy > kd[3]) di1 = (qy - kd[3]) * (qy - kd[3]), dsq += di1;
  double worst = DBL_MAX, ans = b.cloud_depth[(size_t)p * mc];
  // the current root-to-leaf path: bit l set = the FAR child was taken at level l (its near child is done); levels >= plen: near
  unsigned long long path0 = 0;
  unsigned long long pathx[KD_MAXW];  // levels 64 .. (touched only by trees deeper than 64: private memory); words [0, nx) are in use
  int plen = 0, nx = 0;
  auto bit = [&](int l) -> bool { return l < 64 ? (path0 >> l) & 1ull : (pathx[min(l >> 6, KD_MAXW) - 1] >> (l & 63)) & 1ull; };
  for (;;) {
    // down: along the recorded path, then near children to a leaf
    int node = 0, lvl = 0;
    double mind = dsq, d0 = di0, d1 = di1;
    KdNode nd = nodes[0];
    while (nd.feat >= 0) {
      const double val = nd.feat ? qy : qx;
      const bool near1 = (val - nd.lo) + (val - nd.hi) < 0.0;
      if (lvl < plen && bit(lvl)) {
        const double cut = near1 ? (val - nd.hi) * (val - nd.hi) : (val - nd.lo) * (val - nd.lo);
        const double dst = nd.feat ? d1 : d0;
        mind = mind + cut - dst;
        if (nd.feat) d1 = cut; else d0 = cut;
        node = near1 ? nd.b : nd.a;
      } else {
        node = near1 ? nd.a : nd.b;
      }
      lvl++;
      nd = nodes[node];
    }
    // the leaf: points in index-array order against the worst distance at entry; a strictly smaller distance replaces
    {
      const int cnt = nd.b - nd.a;
      if (W == 1) {
        const double wl = worst;
        for (int i = 0; i < cnt; i++) {
          const double dx = qx - pxy[2 * (nd.a + i)], dy = qy - pxy[2 * (nd.a + i) + 1];
          const double d = dx * dx + dy * dy;
          if (d < wl && d < worst) worst = d, ans = pdep[nd.a + i];
        }
      } else {
        const bool in = gl < cnt;
        const int q = nd.a + min(gl, max(cnt - 1, 0));
        const double dx = qx - pxy[2 * q], dy = qy - pxy[2 * q + 1];
        const double d = dx * dx + dy * dy;
        double bd = (in && d < worst) ? d : DBL_MAX;
        int bi = (in && d < worst) ? gl : 1 << 20;
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1) {
          const double od = __shfl_xor(bd, o, 64);
          const int ob = __shfl_xor(bi, o, 64);
          if (ob < (1 << 20) && (bi >= (1 << 20) || od < bd || (od == bd && ob < bi))) bd = od, bi = ob;
        }
        if (bi < (1 << 20)) worst = bd, ans = pdep[nd.a + bi];
      }
    }
    // up: the deepest level of the path whose far child is still pending and passes mindistsq <= worst (the others below it fail
    // now, which is when the recursion would test them)
    int take = -1;
    {
      int node2 = 0;
      double mind2 = dsq, e0 = di0, e1 = di1;
      for (int l2 = 0; l2 < lvl; l2++) {
        const KdNode m = nodes[node2];
        const double val = m.feat ? qy : qx;
        const bool near1 = (val - m.lo) + (val - m.hi) < 0.0;
        const double cut = near1 ? (val - m.hi) * (val - m.hi) : (val - m.lo) * (val - m.lo);
        const double mo = mind2 + cut - (m.feat ? e1 : e0);
        if (l2 < plen && bit(l2)) {
          mind2 = mo;
          if (m.feat) e1 = cut; else e0 = cut;
          node2 = near1 ? m.b : m.a;
        } else {
          if (mo <= worst) take = l2;
          node2 = near1 ? m.a : m.b;
        }
      }
    }
    if (take < 0) break;
    if (take < 64) {
      path0 = (path0 & ((1ull << take) - 1ull)) | (1ull << take);
      nx = 0;
    } else {
      const int w = min(take >> 6, KD_MAXW) - 1;
      while (nx <= w) pathx[nx++] = 0ull;
      pathx[w] = (pathx[w] & ((1ull << (take & 63)) - 1ull)) | (1ull << (take & 63));
      nx = w + 1;
    }
    plen = take + 1;
  }
  return ans;
}
