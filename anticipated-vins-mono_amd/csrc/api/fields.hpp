// api/fields.hpp - the descriptor tables of the ABI structs' arrays

namespace {
// ---- the arrays of the ABI structs, and how they travel ----
// One descriptor per array: where its pointer sits in the struct, how many elements it has for the struct's dims, and which entry points
// read it (in) and return it to the caller (out).  Every size is written here once; staging, packing and the copies back walk the tables.
struct Field {
  const char* pool;                                  // its staging buffer in the ctx's pool
  size_t offset, elem;                               // the pointer member in the struct; bytes per element
  size_t (*count)(const void* s, const void* dims);  // elements; dims: the batch struct the sizes of an output struct come from (else s itself)
  unsigned in, out;                                  // masks of U_*
  size_t bytes(const void* s, const void* dims) const { return elem * count(s, dims); }
};
struct Table {
  const Field* first;
  size_t n;
  const Field* begin() const { return first; }
  const Field* end() const { return first + n; }
};
template <size_t N>
constexpr Table table_of(const Field (&f)[N]) {
  return {f, N};
}
inline void* get_ptr(const void* s, const Field& f) {
  void* p;
  std::memcpy(&p, static_cast<const char*>(s) + f.offset, sizeof p);
  return p;
}
inline void set_ptr(void* s, const Field& f, const void* p) { std::memcpy(static_cast<char*>(s) + f.offset, &p, sizeof p); }

// who uses an array: the calls that take the whole batch (solve, pre-integration, factor evaluation; struct-valued outputs), and the ones
// that take a subset of the window tables (U_KEYF: the keyframe decision, U_FAIL: the failure detection; the feature manager's calls -
// U_TRK: the track tables of a window with its depths and td rows - and the image appended to them -, U_DEPTH: setDepth, U_PUSH: the raw
// IMU samples, U_SLIDE_TD: the td rows beside U_SLIDE in avm_slide_window_tracks; avm_fsel_select_image_batch - U_SELECT: what travels in,
// U_SELECT_BACK: what it writes and returns; the relocalization's calls - U_RELO_SET: avm_set_relo_frame_batch, U_RELO_RESOLVE:
// avm_relo_resolve_batch, U_RELO_FINISH: avm_relo_finish_batch; U_KEEP: avm_prior_keep_batch)
enum : unsigned { U_WHOLE = 1, U_TRI = 2, U_SLIDE = 4, U_PROP = 8, U_CLOUD = 16, U_ALIGN = 32, U_KEYF = 64, U_FAIL = 128,
                  U_TRK = 256, U_DEPTH = 512, U_PUSH = 1024, U_SLIDE_TD = 2048, U_SELECT = 4096, U_SELECT_BACK = 8192,
                  U_RELO_SET = 16384, U_RELO_RESOLVE = 32768, U_RELO_FINISH = 65536, U_KEEP = 131072, U_SFM = 262144 };
constexpr unsigned U_GEOM = U_WHOLE | U_TRI | U_SLIDE | U_CLOUD, U_IMU = U_WHOLE | U_SLIDE | U_PROP;

// S: the struct of the member; D, nmember: the struct the dims come from (`d` in `count`) and its batch size (`N` in `count`)
#define FIELD(S, D, nmember, pool, member, type, count, in, out)                                                              \
  {pool, offsetof(S, member), sizeof(type),                                                                                   \
   [](const void* sp, const void* dp) -> size_t {                                                                             \
     static_assert(std::is_same<std::remove_cv_t<std::remove_pointer_t<decltype(S::member)>>, type>::value, #member);         \
     const S& s = *static_cast<const S*>(sp);                                                                                 \
     const D& d = *static_cast<const D*>(dp);                                                                                 \
     const size_t N = d.nmember;                                                                                              \
     return count;                                                                                                            \
   },                                                                                                                         \
   in, out},

// avm_window_batch.  The four state arrays come first so that the packed path can bring them back with one copy (N_STATES).
#define WIN(member, type, count, in, out) FIELD(avm_window_batch, avm_window_batch, n_windows, "w_" #member, member, type, count, in, out)
const Field WINDOW_FIELDS[] = {
    WIN(pose, double, N * 77, U_GEOM | U_PROP | U_ALIGN | U_FAIL | U_RELO_SET | U_RELO_FINISH, U_WHOLE | U_SLIDE | U_PROP | U_ALIGN)
    WIN(speedbias, double, N * 99, U_IMU | U_ALIGN | U_FAIL, U_WHOLE | U_SLIDE | U_PROP | U_ALIGN)
    WIN(ex_pose, double, N * 7, U_GEOM | U_ALIGN | U_SFM, U_WHOLE | U_SLIDE)
    WIN(inv_depth, double, N * d.max_feat, U_GEOM | U_ALIGN | U_TRK | U_DEPTH, U_WHOLE | U_TRI | U_SLIDE | U_ALIGN | U_TRK | U_DEPTH)
    WIN(n_feat, int32_t, N, U_GEOM | U_ALIGN | U_SFM | U_KEYF | U_TRK | U_DEPTH | U_RELO_RESOLVE, U_SLIDE | U_TRK)
    WIN(feat_start, int32_t, N * d.max_feat, U_GEOM | U_ALIGN | U_SFM | U_KEYF | U_TRK | U_RELO_RESOLVE, U_SLIDE | U_TRK)
    WIN(feat_nobs, int32_t, N * d.max_feat, U_WHOLE | U_TRI | U_SLIDE | U_ALIGN | U_SFM | U_KEYF | U_TRK, U_SLIDE | U_TRK)
    WIN(feat_obs_begin, int32_t, N * d.max_feat, U_GEOM | U_ALIGN | U_SFM | U_KEYF | U_TRK, U_SLIDE | U_TRK)
    WIN(obs_xy, double, N * d.max_obs * 2, U_GEOM | U_ALIGN | U_SFM | U_KEYF | U_TRK, U_SLIDE | U_TRK)
    WIN(imu_n, int32_t, N * 10, U_IMU | U_PUSH, U_SLIDE | U_PUSH)
    WIN(imu_dt, double, N * 10 * d.max_samp, U_IMU | U_PUSH, U_SLIDE | U_PUSH)
    WIN(imu_acc, double, N * 10 * (d.max_samp + 1) * 3, U_IMU | U_PUSH, U_SLIDE | U_PUSH)
    WIN(imu_gyr, double, N * 10 * (d.max_samp + 1) * 3, U_IMU | U_PUSH, U_SLIDE | U_PUSH)
    WIN(imu_lin_ba, double, N * 30, U_WHOLE | U_SLIDE, U_SLIDE)
    WIN(imu_lin_bg, double, N * 30, U_WHOLE | U_SLIDE, U_SLIDE)
    WIN(prior_n, int32_t, N, U_WHOLE | U_KEEP, 0)
    WIN(prior_nblk, int32_t, N, U_WHOLE | U_KEEP, 0)
    WIN(prior_blk_kind, int32_t, N * d.max_pblk, U_WHOLE | U_KEEP, 0)
    WIN(prior_blk_frame, int32_t, N * d.max_pblk, U_WHOLE | U_KEEP, 0)
    WIN(prior_J, double, N * d.max_prior * d.max_prior, U_WHOLE | U_KEEP, 0)
    WIN(prior_r, double, N * d.max_prior, U_WHOLE | U_KEEP, 0)
    WIN(prior_x0, double, N * d.max_pblk * 9, U_WHOLE | U_KEEP, 0)
    WIN(obs_vel_td, double, N * d.max_obs * 4, U_WHOLE | U_TRK | U_SLIDE_TD, U_TRK | U_SLIDE_TD)
    WIN(td, double, N, U_WHOLE, U_WHOLE)  // para_Td: in/out
    WIN(relo_n, int32_t, N, U_WHOLE, 0)
    WIN(relo_frame, int32_t, N, U_WHOLE, 0)
    WIN(relo_feat, int32_t, N * d.max_feat, U_WHOLE, 0)
    WIN(relo_xy, double, N * d.max_feat * 2, U_WHOLE, 0)
    WIN(relo_pose, double, N * 7, U_WHOLE, U_WHOLE)  // relo_Pose: in/out
    WIN(failure_occur, int32_t, N, U_WHOLE, 0)
    WIN(last_pose0, double, N * 7, U_WHOLE, 0)};
#undef WIN
constexpr Table WINDOWS = table_of(WINDOW_FIELDS);
constexpr int N_STATES = 4;  // pose | speedbias | ex_pose | inv_depth

// avm_prior_out of a batch (one device block "po_pack" in host mode: one memset, and for small batches one copy back); avm_prior_keep_batch
// rewrites slots of it in place: there it travels both ways
#define PO(member, type, count) FIELD(avm_prior_out, avm_window_batch, n_windows, "po_" #member, member, type, count, U_KEEP, U_WHOLE | U_KEEP)
const Field PRIOR_OUT_FIELDS[] = {
    PO(n, int32_t, N) PO(nblk, int32_t, N) PO(blk_kind, int32_t, N * s.max_pblk) PO(blk_frame, int32_t, N * s.max_pblk)
    PO(J, double, N * s.max_prior * s.max_prior) PO(r, double, N * s.max_prior) PO(x0, double, N * s.max_pblk * 9)};
#undef PO
constexpr Table PRIOR_OUT = table_of(PRIOR_OUT_FIELDS);

// avm_fsel_batch (FSW: the members the split of avm_fsel_select_image_batch writes)
#define FS(member, type, count) FIELD(avm_fsel_batch, avm_fsel_batch, n_problems, "f_" #member, member, type, count, U_WHOLE, 0)
#define FSW(member, type, count) FIELD(avm_fsel_batch, avm_fsel_batch, n_problems, "f_" #member, member, type, count, U_WHOLE, U_SELECT_BACK)
const Field FSEL_FIELDS[] = {
    FS(hor_pos, double, N * (d.horizon + 1) * 3) FS(hor_quat, double, N * (d.horizon + 1) * 4) FS(nr_imu, int32_t, N) FS(delta_imu, double, N)
    FSW(n_cand, int32_t, N) FSW(cand_id, int32_t, N * d.max_cand) FSW(cand_xy, double, N * d.max_cand * 2) FSW(cand_prob, double, N * d.max_cand)
    FSW(n_used, int32_t, N) FSW(used_id, int32_t, N * d.max_used) FSW(used_xy, double, N * d.max_used * 2)
    FS(n_cloud, int32_t, N) FS(cloud_xy, double, N * d.max_cloud * 2) FS(cloud_depth, double, N * d.max_cloud)};
#undef FS
#undef FSW
constexpr Table FSEL = table_of(FSEL_FIELDS);

#define FO(pool, member, type) FIELD(avm_fsel_out, avm_fsel_batch, n_problems, pool, member, type, N * d.max_features, 0, U_WHOLE)
const Field FSEL_OUT_FIELDS[] = {FIELD(avm_fsel_out, avm_fsel_batch, n_problems, "fo_n", n_selected, int32_t, N, 0, U_WHOLE)
                                 FO("fo_ids", selected_ids, int32_t) FO("fo_fv", fvalues, double) FO("fo_gap", min_gap, double)};
#undef FO
constexpr Table FSEL_OUT = table_of(FSEL_OUT_FIELDS);

#define TD(member, per) FIELD(avm_td_factor_batch, avm_td_factor_batch, n, "td_" #member, member, double, N * per, U_WHOLE, 0)
const Field TD_FIELDS[] = {TD(pose_i, 7) TD(pose_j, 7) TD(ex_pose, 7) TD(inv_depth, 1) TD(td, 1) TD(pts_i, 2) TD(pts_j, 2)
                           TD(vel_i, 2) TD(vel_j, 2) TD(td_i, 1) TD(td_j, 1) TD(row_i, 1) TD(row_j, 1)};
#undef TD
constexpr Table TD_FACTORS = table_of(TD_FIELDS);

#define HZ(member, type, per) FIELD(avm_fsel_horizon_in, avm_fsel_horizon_in, n_problems, "h_" #member, member, type, N * per, U_WHOLE, 0)
const Field HORIZON_FIELDS[] = {HZ(k_pos, double, 3) HZ(k_quat, double, 4) HZ(k_ba, double, 3) HZ(k1_pos, double, 3) HZ(k1_vel, double, 3)
                                HZ(k1_quat, double, 4) HZ(acc, double, 3) HZ(gyr, double, 3) HZ(nr_imu, int32_t, 1) HZ(delta_imu, double, 1)};
#undef HZ
constexpr Table HORIZON_IN = table_of(HORIZON_FIELDS);

// avm_align_batch / avm_align_out (avm_visual_initial_align_batch)
#define AL(member, type, count) FIELD(avm_align_batch, avm_align_batch, n_windows, "al_" #member, member, type, count, U_WHOLE, 0)
const Field ALIGN_FIELDS[] = {
    AL(n_frames, int32_t, N) AL(frame_R, double, N * d.max_frames * 9) AL(frame_T, double, N * d.max_frames * 3) AL(tic, double, N * 3)
    AL(imu_n, int32_t, N * (d.max_frames - 1)) AL(imu_dt, double, N * (d.max_frames - 1) * d.max_samp)
    AL(imu_acc, double, N * (d.max_frames - 1) * (d.max_samp + 1) * 3) AL(imu_gyr, double, N * (d.max_frames - 1) * (d.max_samp + 1) * 3)
    AL(imu_lin_ba, double, N * (d.max_frames - 1) * 3) AL(imu_lin_bg, double, N * (d.max_frames - 1) * 3) AL(key_index, int32_t, N * AVM_NFRAMES)};
#undef AL
constexpr Table ALIGN = table_of(ALIGN_FIELDS);
#define AO(member, type, count) FIELD(avm_align_out, avm_align_batch, n_windows, "ao_" #member, member, type, count, 0, U_WHOLE)
const Field ALIGN_OUT_FIELDS[] = {AO(ok, int32_t, N) AO(delta_bg, double, N * 3) AO(g_c0, double, N * 3) AO(x, double, N * (3 * d.max_frames + 1))
                                  AO(g_world, double, N * 3) AO(deltas, double, N * (d.max_frames - 1) * 10)};
#undef AO
constexpr Table ALIGN_OUT = table_of(ALIGN_OUT_FIELDS);

// avm_sfm_batch / avm_sfm_out (avm_global_sfm_batch).  The outputs travel both ways: a stream writes only the rows its ok allows, the
// others return as the caller passed them.  SfmDims: the three sizes the outputs' extents come from (two structs hold them)
struct SfmDims {
  int32_t n_windows, max_frames, max_feat;
};
#define SF(member, type, count) FIELD(avm_sfm_batch, avm_sfm_batch, n_windows, "sf_" #member, member, type, count, U_WHOLE, 0)
const Field SFM_FIELDS[] = {SF(l, int32_t, N) SF(n_frames, int32_t, N) SF(key_index, int32_t, N * AVM_NFRAMES) SF(frame_n_pts, int32_t, N * d.max_frames)
                            SF(frame_pt_id, int32_t, N * d.max_frames * d.max_pts) SF(relative_R, double, N * 9) SF(relative_T, double, N * 3)
                            SF(frame_pt_xy, double, N * d.max_frames * d.max_pts * 2)};
#undef SF
constexpr Table SFM = table_of(SFM_FIELDS);
#define SO(member, type, count) FIELD(avm_sfm_out, SfmDims, n_windows, "sfo_" #member, member, type, count, U_WHOLE, U_WHOLE)
const Field SFM_OUT_FIELDS[] = {SO(ok, int32_t, N) SO(frame_R, double, N * d.max_frames * 9) SO(frame_T, double, N * d.max_frames * 3)
                                SO(q, double, N * AVM_NFRAMES * 4) SO(T, double, N * AVM_NFRAMES * 3) SO(point, double, N * d.max_feat * 3)
                                SO(point_state, int32_t, N * d.max_feat) SO(ba_counts, int32_t, N * 3) SO(ba_cost, double, N * 2)
                                SO(pnp_q, double, N * AVM_NFRAMES * 4) SO(pnp_t, double, N * AVM_NFRAMES * 3)};
#undef SO
constexpr Table SFM_OUT = table_of(SFM_OUT_FIELDS);
static_assert(sizeof(avm_sfm_batch) == offsetof(avm_sfm_batch, l) + SFM.n * sizeof(void*), "SFM names every array of avm_sfm_batch");
static_assert(sizeof(avm_sfm_out) == SFM_OUT.n * sizeof(void*), "SFM_OUT names every array of avm_sfm_out");

// avm_image_batch: the image of avm_add_image_batch (pools "ai_" ...), the image and image_out of avm_fsel_select_image_batch ("si_" ...,
// "so_" ...: the prefix of on_device), and that call's avm_select_state, whose batch size is the image's
#define IM(pool, member, type, count) FIELD(avm_image_batch, avm_image_batch, n_windows, pool, member, type, count, U_TRK | U_SELECT, U_SELECT_BACK)
const Field IMAGE_FIELDS[] = {IM("n_pts", n_pts, int32_t, N) IM("ids", feature_id, int32_t, N * d.max_pts) IM("xy", xy, double, N * d.max_pts * 2)
                              IM("vel_td", vel_td, double, N * d.max_pts * 4)};
#undef IM
constexpr Table IMAGE = table_of(IMAGE_FIELDS);
#define SS(pool, member, count) FIELD(avm_select_state, avm_image_batch, n_windows, pool, member, int32_t, count, U_SELECT, U_SELECT_BACK)
const Field SELECT_STATE_FIELDS[] = {SS("ss_last", last_feature_id, N) SS("ss_n", n_tracked, N) SS("ss_ids", tracked_id, N * s.max_tracked)
                                     SS("ss_first", first_image, N)};
#undef SS
constexpr Table SELECT_STATE = table_of(SELECT_STATE_FIELDS);
// avm_relo_msg_batch and avm_relo_state (the state's batch size is the windows'); which of the three calls reads / returns a member
#define RM(member, type, count) FIELD(avm_relo_msg_batch, avm_relo_msg_batch, n_windows, "rm_" #member, member, type, count, U_RELO_SET, 0)
const Field RELO_MSG_FIELDS[] = {RM(has_msg, int32_t, N) RM(frame_stamp, double, N) RM(n_match, int32_t, N) RM(match_id, int32_t, N * d.max_match)
                                 RM(match_xy, double, N * d.max_match * 2) RM(prev_relo_t, double, N * 3) RM(prev_relo_q, double, N * 4)};
#undef RM
constexpr Table RELO_MSG = table_of(RELO_MSG_FIELDS);
#define RS(member, type, count, in, out) FIELD(avm_relo_state, avm_window_batch, n_windows, "rs_" #member, member, type, count, in, out)
constexpr unsigned U_RELO_ALL = U_RELO_SET | U_RELO_RESOLVE | U_RELO_FINISH;
const Field RELO_STATE_FIELDS[] = {
    RS(relocalization_info, int32_t, N, U_RELO_ALL, U_RELO_SET | U_RELO_FINISH) RS(relo_frame, int32_t, N, U_RELO_ALL, U_RELO_SET)
    RS(relo_stamp, double, N, U_RELO_SET, U_RELO_SET) RS(n_match, int32_t, N, U_RELO_SET | U_RELO_RESOLVE, U_RELO_SET)
    RS(match_id, int32_t, N * s.max_match, U_RELO_SET | U_RELO_RESOLVE, U_RELO_SET)
    RS(match_xy, double, N * s.max_match * 2, U_RELO_SET | U_RELO_RESOLVE, U_RELO_SET)
    RS(prev_relo_t, double, N * 3, U_RELO_SET | U_RELO_FINISH, U_RELO_SET) RS(prev_relo_q, double, N * 4, U_RELO_SET | U_RELO_FINISH, U_RELO_SET)
    RS(relo_pose, double, N * 7, U_RELO_SET | U_RELO_FINISH, U_RELO_SET)
    RS(drift_correct_yaw, double, N, U_RELO_FINISH, U_RELO_FINISH) RS(drift_correct_t, double, N * 3, U_RELO_FINISH, U_RELO_FINISH)
    RS(relo_relative_t, double, N * 3, U_RELO_FINISH, U_RELO_FINISH) RS(relo_relative_q, double, N * 4, U_RELO_FINISH, U_RELO_FINISH)
    RS(relo_relative_yaw, double, N, U_RELO_FINISH, U_RELO_FINISH)};
#undef RS
constexpr Table RELO_STATE = table_of(RELO_STATE_FIELDS);
// (no pointer member the tables lack: the scalar header, then one pointer per field)
static_assert(sizeof(avm_image_batch) == offsetof(avm_image_batch, n_pts) + IMAGE.n * sizeof(void*), "IMAGE names every array of avm_image_batch");
static_assert(sizeof(avm_select_state) == offsetof(avm_select_state, last_feature_id) + SELECT_STATE.n * sizeof(void*),
              "SELECT_STATE names every array of avm_select_state");
static_assert(sizeof(avm_relo_msg_batch) == offsetof(avm_relo_msg_batch, has_msg) + RELO_MSG.n * sizeof(void*), "RELO_MSG names every array of avm_relo_msg_batch");
static_assert(sizeof(avm_relo_state) == offsetof(avm_relo_state, relocalization_info) + RELO_STATE.n * sizeof(void*),
              "RELO_STATE names every array of avm_relo_state");
}  // namespace
