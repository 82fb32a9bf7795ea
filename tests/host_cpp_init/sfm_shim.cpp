// Test hooks around avm_host::Estimator::initialStructure (include/avm_host.hpp).  The members are filled by the hooks of
// tests/host_cpp/align_shim.cpp (as_load: all_image_frame, Headers, the window), which this file compiles in as they are; the hooks
// below add what initialStructure reads beside them - the features' ids and every frame's points - and run the call.
// Test infrastructure only - the product is the header.
#include "../host_cpp/align_shim.cpp"

extern "C" {

// stream w of the batch: feature ids onto f_manager.feature (list order), the points of every frame into all_image_frame
int ss_load_images(void* hp, const avm_sfm_batch* s, const int32_t* feat_id, int max_feat, int w) {
  Host& H = *static_cast<Host*>(hp);
  return guarded([&] {
    Estimator& E = H.est;
    size_t e = 0;
    for (auto& f : E.f_manager.feature) f.feature_id = feat_id[(size_t)w * max_feat + e++];
    size_t k = 0;
    for (auto it = E.all_image_frame.begin(); it != E.all_image_frame.end(); ++it, ++k) {
      const size_t row = (size_t)w * s->max_frames + k;
      it->second.points.clear();
      for (int n = 0; n < s->frame_n_pts[row]; n++)
        it->second.points[s->frame_pt_id[row * s->max_pts + n]] = {s->frame_pt_xy[(row * s->max_pts + n) * 2], s->frame_pt_xy[(row * s->max_pts + n) * 2 + 1]};
    }
  });
}

// bool Estimator::initialStructure(l, relative_R, relative_T); result[0] receives it, result[1] the SfM's ok
int ss_initial_structure(void* hp, int l, const double* relative_R, const double* relative_T, int32_t* result) {
  Host& H = *static_cast<Host*>(hp);
  return guarded([&] {
    result[0] = H.est.initialStructure(l, relative_R, relative_T) ? 1 : 0;
    result[1] = H.est.sfm_ok;
  });
}

// ImageFrame::R / ::T of every frame, [F][9] / [F][3]
void ss_frames(void* hp, double* frame_R, double* frame_T) {
  Host& H = *static_cast<Host*>(hp);
  size_t k = 0;
  for (auto it = H.est.all_image_frame.begin(); it != H.est.all_image_frame.end(); ++it, ++k) {
    std::copy(it->second.R.begin(), it->second.R.end(), frame_R + 9 * k);
    std::copy(it->second.T.begin(), it->second.T.end(), frame_T + 3 * k);
  }
}
}
