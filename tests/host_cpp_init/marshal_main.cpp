// TEST INFRASTRUCTURE.  A stand-alone program around avm_host::marshal_sfm and the host rule function of avm_global_sfm_batch's table
// check, for the address / undefined-behaviour sanitizers; nothing of HIP and nothing of the library is linked.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DSFM_HD=inline -I include marshal_main.cpp -o marshal_main
//   marshal_main CASE.bin [CASE.bin ...]
// Every argument is one stream written by tests/test_global_sfm_marshal_cpu.py; they are marshalled one after the other through the SAME
// SfmTables object (a large stream, a small one, a large one again), checked by the rules, handed to a stub that stands in for the
// entry point and writes every output array to its full declared extent, and the marshalled tables are dumped to CASE.bin.out.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "avm_host.hpp"
#include "../../anticipated-vins-mono_amd/csrc/sfm/rules.hpp"

using namespace avm_host;

namespace {
template <class T>
std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short read\n");
    std::exit(2);
  }
  return v;
}
template <class T>
void put(FILE* f, const std::vector<T>& v) {
  std::fwrite(v.data(), sizeof(T), v.size(), f);
}

// what the entry point may touch at most: every output to the extent the structs declare
int stub_global_sfm_batch(const avm_sfm_batch* s, const avm_window_batch* w, const int32_t* feat_id, avm_sfm_out* o) {
  for (int b = 0; b < s->n_windows; b++)
    if (const int rule = avm::check_sfm_tables(*s, b)) return 8 * b + rule;
  const size_t B = s->n_windows, MF = s->max_frames, MFE = w->max_feat;
  long sum = 0;
  for (size_t i = 0; i < B * MFE; i++) sum += feat_id[i];
  for (size_t i = 0; i < B; i++) o->ok[i] = 0;
  for (size_t i = 0; i < B * MF * 9; i++) o->frame_R[i] = 1.0 + (double)(sum % 7);
  for (size_t i = 0; i < B * MF * 3; i++) o->frame_T[i] = 2.0;
  for (size_t i = 0; i < B * 44; i++) o->q[i] = o->pnp_q[i] = 3.0;
  for (size_t i = 0; i < B * 33; i++) o->T[i] = o->pnp_t[i] = 4.0;
  for (size_t i = 0; i < B * MFE * 3; i++) o->point[i] = 5.0;
  for (size_t i = 0; i < B * MFE; i++) o->point_state[i] = 1;
  for (size_t i = 0; i < B * 3; i++) o->ba_counts[i] = 6;
  for (size_t i = 0; i < B * 2; i++) o->ba_cost[i] = 7.0;
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  SfmTables t;  // one object for every stream: a second stream of another size is an ordinary event
  for (int a = 1; a < argc; a++) {
    FILE* f = std::fopen(argv[a], "rb");
    if (!f) return 2;
    const auto h = take<int32_t>(f, 5);
    const int l = h[0], F = h[1], nf = h[2], P = h[3], no = h[4];
    const auto start = take<int32_t>(f, nf), nobs = take<int32_t>(f, nf), obeg = take<int32_t>(f, nf), fid = take<int32_t>(f, nf);
    const auto key = take<int32_t>(f, 11), npts = take<int32_t>(f, F), pid = take<int32_t>(f, (size_t)F * P);
    const auto obs = take<double>(f, (size_t)no * 2), pxy = take<double>(f, (size_t)F * P * 2);
    const auto relR = take<double>(f, 9), relT = take<double>(f, 3), ex = take<double>(f, 7);
    std::fclose(f);
    // the members initialStructure reads
    std::list<FeaturePerId> feature;
    for (int e = 0; e < nf; e++) {
      FeaturePerId fp(fid[e], start[e]);
      for (int k = 0; k < nobs[e]; k++) {
        FeaturePerFrame pf;
        pf.point = {obs[2 * (size_t)(obeg[e] + k)], obs[2 * (size_t)(obeg[e] + k) + 1], 1.0};
        fp.feature_per_frame.push_back(pf);
      }
      feature.push_back(fp);
    }
    std::map<double, ImageFrame> frames;
    double Headers[AVM_NFRAMES];
    for (int k = 0; k < F; k++) {
      ImageFrame fr;
      for (int n = 0; n < npts[k]; n++) fr.points[pid[(size_t)k * P + n]] = {pxy[((size_t)k * P + n) * 2], pxy[((size_t)k * P + n) * 2 + 1]};
      frames[100.0 + 0.05 * k] = fr;
    }
    for (int i = 0; i < AVM_NFRAMES; i++) Headers[i] = 100.0 + 0.05 * key[i];
    marshal_sfm(feature, frames, Headers, l, relR.data(), relT.data(), ex.data(), t);
    const avm_sfm_batch sb = t.batch();
    const avm_window_batch fb = t.full();
    avm_sfm_out so = t.out();
    const int rc = stub_global_sfm_batch(&sb, &fb, t.feat_id.data(), &so);
    std::printf("%s: n_feat %d n_frames %d max_pts %d max_obs %d rc %d ok %d\n", argv[a], t.n_feat, t.n_frames, t.max_pts, t.max_obs, rc, t.ok);
    if (rc != 0 || t.ok != 0) return 3;
    FILE* o = std::fopen((std::string(argv[a]) + ".out").c_str(), "wb");
    if (!o) return 2;
    put(o, std::vector<int32_t>{t.l, t.n_frames, t.n_feat, t.max_pts, t.max_obs});
    put(o, t.feat_start), put(o, t.feat_nobs), put(o, t.feat_obs_begin), put(o, t.feat_id), put(o, t.key_index), put(o, t.frame_n_pts), put(o, t.frame_pt_id);
    put(o, t.obs_xy), put(o, t.frame_pt_xy), put(o, t.relative_R), put(o, t.relative_T), put(o, t.ex_pose);
    std::fclose(o);
  }
  return 0;
}
