// Host functions that cross a translation unit, grouped by the .hip that defines them; capi.hip (and, where noted,
// another .hip) calls them.  Every defining file includes this header, so a definition sits under the eye of its
// declaration; one that drifts from it is a second overload, and the library no longer loads (unresolved symbol).
#pragma once
#include "common.hpp"

namespace miso {

struct AlignK;    // align.hpp
struct PairSdfK;  // pair_stage.hpp
struct GradPlan;  // grad_plan.hpp (with plan_grad, the host-side plan of a binned call's grid gradient)
struct PullBatch;

// ---- encode.hip
hipError_t launch_encode_fwd(const GridK& g, bool vec4, const float* x, int64_t n, float* out, int64_t ld,
                             const int* perm, hipStream_t s);
hipError_t launch_encode_bwd(const GridK& g, bool vec4, const float* x, int64_t n, const float* gf, int64_t ld,
                             float* gx, const int* perm, hipStream_t s);
hipError_t launch_encode_bwd2(const GridK& g, bool vec4, const float* x, int64_t n, const float* gf, int64_t ld,
                              const float* ggx, float* ggo, int64_t ldgg, float* gx, const int* perm, hipStream_t s);

// ---- sdf_fused.hip
bool fused_shape_supported(int C, int L, int H, int NH);
int64_t mlp_packed_floats(int F, int H, int NH);
hipError_t launch_mlp_pack(const MlpK& m, int F, int H, int NH, float* out, hipStream_t s);
hipError_t launch_sdf_fwd(int C, int L, int H, int NH, const GridK& g, const float* packed, const float* x, int64_t n,
                          float* sdf, uint32_t* mask, const int* perm, const LossInK& lin, hipStream_t s);
hipError_t launch_sdf_bwd(int C, int L, int H, int NH, const GridK& g, const float* packed, const float* x, int64_t n,
                          const float* gsdf, const uint32_t* mask, float* gx, bool want_grid, const int* perm,
                          float* dfeat_out, uint32_t defer_mask, bool gsdf_sorted, hipStream_t s);

// ---- decoder_wgrad.hip (sdf_wgrad_workspace_floats: 0 = shape not covered, or an empty batch)
int64_t sdf_wgrad_workspace_floats(int C, int L, int H, int NH, int64_t n);
hipError_t launch_sdf_wgrad(int C, int L, int H, int NH, const GridK& g, const float* packed, const float* x, int64_t n,
                            const float* gsdf, const uint32_t* mask, const int* perm, bool gsdf_sorted,
                            const WgradOutK& out, float* workspace, hipStream_t s);

// ---- sdf_train.hip (sdf_train_lds_bytes: 0 = shape not covered, or its widest launch does not fit a workgroup's LDS)
int64_t sdf_train_lds_bytes(int C, int L, int H, int NH, bool scat);
hipError_t launch_sdf_train(int C, int L, int H, int NH, const GridK& g, const float* packed, const float* x, int64_t n,
                            float* sdf, const int* perm, const LossInK& lin, float* dfeat_out, uint32_t defer_mask,
                            bool scat, hipStream_t s);

// ---- atlas.hip
hipError_t launch_atlas_sdf(int C, int L, int H, int NH, const AtlasK& a, const float* packed, bool exact, hipStream_t s);

// ---- atlas_bwd.hip (atlas_bwd_covered: shape in the kernel table and its launch fits a workgroup's LDS, both arithmetics)
int64_t atlas_bwd_workspace_bytes(int64_t n, int n_submaps);
bool atlas_bwd_covered(int C, int L, int H, int NH, int n_submaps, bool poses);
hipError_t launch_atlas_sdf_bwd(int C, int L, int H, int NH, const AtlasK& a, const float* packed, const float* gsdf,
                                float* gx, float* gposes, float* workspace, bool exact, hipStream_t s);

// ---- trace.hip
hipError_t launch_atlas_trace(int C, int L, int H, int NH, const AtlasK& a, const TraceK& t, const float* packed, bool exact,
                              hipStream_t s);

// ---- sort.hip
int64_t sort_workspace_bytes(int64_t n, int tiles);
hipError_t launch_sort(const GridK& g, const float* x, int64_t n, int tiles, void* ws, float* xs, float* xn, int* perm,
                       int* tile_off, hipStream_t s);

// ---- grad_pull.hip (zero_level_grads: the gradient buffers of `levels`, cleared by kernels)
int64_t pull_queue_ints(int64_t n);
hipError_t zero_level_grads(const GridK& g, uint32_t levels, hipStream_t s);
hipError_t launch_grad_pull(const GridK& g, const GradPlan& plan, const PullBatch& batch, hipStream_t s);

// ---- grad_pull_mc.hip (called by launch_grad_pull for a plan of form PULL_MC)
hipError_t launch_grad_pull_mc(const GridK& g, const GradPlan& plan, const PullBatch& batch, hipStream_t s);

// ---- pair_latent.hip (launch_pair_batch: called by launch_align_a; sdf != nullptr: the SDF residual of pair_sdf.hip in
//      place of the latent one, the overlap gate in a launch of its own in front of it)
hipError_t launch_src_boxes(const float* p, int64_t n, float* boxes, hipStream_t s);
hipError_t launch_overlap_count(const float* pose, const float* p, int64_t n, const float* bmin, const float* bmax,
                                float* out, hipStream_t s);
hipError_t launch_pair_latent(const GridK& g, bool vec4, const float* pose, const float* p, const float* fsrc, int64_t ld,
                              int64_t n, int loss_type, double* out, hipStream_t s);
hipError_t launch_pair_batch(const AlignPairK* plan_dev, int n_pairs, int64_t max_n, int64_t max_gate_n, bool vec4,
                             const float* pose_all, int loss_type, double* out_all, float* cnt_all,
                             const int32_t* stopped, int64_t max_gate_rows, const int32_t* order, const PairSdfK* sdf,
                             hipStream_t s);

// ---- pair_sdf.hip (pair_sdf_covered: shape in the kernel table and its launch fits a workgroup's LDS, both arithmetics;
//      launch_pair_sdf_stage: called by launch_pair_batch for a plan whose residual is an SDF one)
bool pair_sdf_covered(int C, int L, int H, int NH);
hipError_t launch_pair_sdf_stage(const PairSdfK& k, const AlignPairK* plan_dev, int n_pairs, int64_t max_n,
                                 const float* pose_all, int loss_type, double* out_all, const int32_t* stopped,
                                 const int32_t* order, hipStream_t s);

// ---- align.hip
hipError_t launch_align_a(const AlignK& k, int64_t max_n, int64_t max_gate_n, int64_t max_gate_rows, bool vec4,
                          bool poses_ready, hipStream_t s);
hipError_t launch_align_b(const AlignK& k, hipStream_t s);

// ---- lm.hip
hipError_t launch_lm_normal_eq(const float* x, const float* R, const float* grad, const float* sdf, const float* gt,
                               int64_t n, int loss_type, float gm_scale, float* out, hipStream_t s);
hipError_t launch_track_loss(const TrackAdamK& k, hipStream_t st);
hipError_t launch_track_tail(const TrackAdamK& k, hipStream_t st);
hipError_t launch_lm_track_head(const LmTrackK& k, hipStream_t s);
hipError_t launch_lm_track_tail(const LmTrackK& k, const float* grad, const float* sdf, int loss_type, float gm_scale,
                                hipStream_t s);

// ---- sample.hip
size_t sample_rays_workspace_bytes(int64_t n_rays, int32_t n_frames);
hipError_t launch_sample_rays(const miso_ray_frames_t& f, const miso_ray_sampling_t& c, const float* lin, int64_t n_rays,
                              const int64_t* pix_b, const int64_t* pix_h, const int64_t* pix_w, const float* u,
                              const float* g, void* workspace, float* coords, int64_t* ids, float* aux, float* pc_world,
                              float* z_vals, int32_t* counts, hipStream_t s);

// ---- adam.hip (launch_adam_step: every flag-driven form -- `when` says where the scalars come from, miso_hip.h)
void adam_scalars_table(double lr, double b1, double b2, double eps, int first_step, int count, float* out);
hipError_t launch_adam_bump(int32_t* step, const float* guard, hipStream_t s);
hipError_t launch_loss_total_bump(const float* slots, int n, float* total, int32_t* step, float* host_ring, int ring_len,
                                  hipStream_t s);
hipError_t launch_adam(float* p, float* g, float* m, float* v, int64_t n, double lr, double b1, double b2, double eps,
                       int step, int zero_grad, hipStream_t s);
hipError_t launch_adam_step(const miso_adam_tensor_t* t, int count, const miso_adam_when_t& when, const float* guard,
                            hipStream_t s);

// ---- loss.hip (launch_zero_words clears n_words 32-bit words with a kernel; see there why not hipMemsetAsync)
hipError_t launch_zero_fill(float* p, int64_t n, hipStream_t s);
hipError_t launch_zero_words(void* p, int n_words, hipStream_t s);
hipError_t launch_mapping_loss(int loss_type, float w_sdf, float w_fs, float trunc, const float* pred, const float* targ,
                               const float* valid, const float* sign, const float* weight, int64_t n, float* gpred,
                               float* gpred_fs, float* loss_out, hipStream_t s);
hipError_t launch_mapping_loss_rows(int loss_type, float w_sdf, float w_fs, float trunc, const float* pred,
                                    const float* rows, int64_t n, float* gpred, float* loss_out, hipStream_t s);

// ---- mcubes.hip
int64_t mc_words(int32_t nx, int32_t ny, int32_t nz);
int64_t mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
void mc_copy_table(int8_t* out);
hipError_t launch_mc_classify(const float* u, int32_t nx, int32_t ny, int32_t nz, float iso, void* workspace,
                              int32_t* counts, hipStream_t s);
hipError_t launch_mc_emit(int32_t nx, int32_t ny, int32_t nz, void* workspace, const int64_t* offsets, int32_t n_listed,
                          int64_t capacity, int64_t* faces, hipStream_t s);
hipError_t launch_mc_vertices(const float* u, int32_t nx, int32_t ny, int32_t nz, float iso, void* workspace,
                              const int64_t* offsets, int32_t n_listed, int64_t capacity, float* verts, hipStream_t s);

// ---- rigid.hip
hipError_t launch_mapping_batch(const float* R, const float* t, int32_t K, const int64_t* table, int64_t table_len,
                                const int64_t* frame_ids, const float* x, const float* target, const void* valid,
                                const float* sign, const float* weight, int64_t n, float* y, float* rows,
                                const int64_t* strides, int valid_is_bool, int sanitize, hipStream_t s);
hipError_t launch_rigid_by_index(const float* R, const float* t, const int64_t* idx, const float* x, int64_t n, int32_t K,
                                 int transpose, float* y, hipStream_t s);

// ---- pool.hip
hipError_t launch_grid_pool_avg(const float* coords, const float* feat, int64_t n, int32_t d, int64_t ld,
                                const float* bmin, float cell, int32_t nx, int32_t ny, int32_t nz, float* acc,
                                int32_t* cnt, hipStream_t s);

// ---- voxel.hip
int64_t voxel_down_workspace_bytes(int64_t capacity);
hipError_t launch_voxel_down_sample(const float* points, int64_t ld, int64_t capacity, const int32_t* n_live, float voxel_size,
                                    void* workspace, int64_t* out_idx, int32_t* out_count, hipStream_t s);
hipError_t launch_voxel_select_rows(const float* src_coords, const int64_t* src_ids, const float* src_aux,
                                    const int64_t* out_idx, const int32_t* out_count, int64_t capacity, float* dst_coords,
                                    int64_t* dst_ids, float* dst_aux, int32_t* live_rows, hipStream_t s);

// ---- nn.hip
int64_t nn_workspace_bytes(const miso_nn_plan_t& plan);
hipError_t launch_nn_build(const miso_nn_plan_t& plan, const float* tgt, int64_t ld, void* workspace, hipStream_t s);
hipError_t launch_nn_query(const miso_nn_plan_t& plan, void* workspace, const float* src, int64_t ld, int64_t n, float* out_d2,
                           int64_t* out_idx, int32_t* stats, hipStream_t s);
hipError_t launch_nn_all_pairs(const float* tgt, int64_t ld_t, int64_t m, const float* src, int64_t ld_s, int64_t n,
                               float* out_d2, int64_t* out_idx, hipStream_t s);
// knn.hip: the k nearest on the same index
hipError_t launch_nn_knn(const miso_nn_plan_t& plan, void* workspace, const float* src, int64_t ld, int64_t n, int k, float* out_d2,
                         int64_t* out_idx, int32_t* stats, hipStream_t s);
hipError_t launch_nn_knn_all_pairs(const float* tgt, int64_t ld_t, int64_t m, const float* src, int64_t ld_s, int64_t n, int k,
                                   float* out_d2, int64_t* out_idx, hipStream_t s);
hipError_t launch_nn_knn_normals(const miso_nn_plan_t& plan, void* workspace, const float* pts, int64_t ld, int64_t n, int k,
                                 float* normals, int32_t* counts, hipStream_t s);

// ---- icp.hip
hipError_t launch_icp_transform(const float* pose, const float* src, int64_t ld, int64_t n, float* out, hipStream_t s);
int64_t icp_workspace_bytes(int64_t n);
hipError_t launch_icp_sums(const float* moved, const float* d2, const int64_t* idx, int64_t n, const float* tgt, int64_t ld_t,
                           int64_t m, const float* normals, int64_t ld_n, double max_dist, int kind, int loss, double tukey_k,
                           const double* origin, void* workspace, double* out, hipStream_t s);
hipError_t launch_nn_normals(const miso_nn_plan_t& plan, const void* workspace, const float* pts, int64_t ld, int64_t n,
                             double radius, float* normals, int32_t* counts, hipStream_t s);

// ---- mesh.hip
int64_t mesh_workspace_bytes(const miso_mesh_plan_t& plan);
hipError_t launch_mesh_count(const miso_mesh_plan_t& plan, const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris,
                             int64_t ld_t, void* workspace, int64_t* entries, hipStream_t s);
hipError_t launch_mesh_build(const miso_mesh_plan_t& plan, void* workspace, int32_t* lists, int64_t capacity, hipStream_t s);
hipError_t launch_mesh_cast_rays(const miso_mesh_plan_t& plan, const void* workspace, const int32_t* lists, int64_t capacity,
                                 const float* org, int64_t ld_o, const float* dir, int64_t ld_d, int64_t n, float t_min, float t_max,
                                 float* out_t, int64_t* out_tri, int64_t* stats, hipStream_t s);
hipError_t launch_mesh_cast_rays_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t,
                                     int64_t n_tri, const float* org, int64_t ld_o, const float* dir, int64_t ld_d, int64_t n,
                                     float t_min, float t_max, float* out_t, int64_t* out_tri, hipStream_t s);

// ---- mesh_sdf.hip (plan_far: null = the fine index only)
hipError_t launch_mesh_closest(const miso_mesh_plan_t& plan, const void* workspace, const int32_t* lists, int64_t capacity,
                               const miso_mesh_plan_t* plan_far, const void* workspace_far, const int32_t* lists_far,
                               int64_t capacity_far, const float* pts, int64_t ld_p, int64_t n, float* out_d2, int64_t* out_tri,
                               float* out_vw, int64_t* stats, hipStream_t s);
hipError_t launch_mesh_closest_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t, int64_t n_tri,
                                   const float* pts, int64_t ld_p, int64_t n, float* out_d2, int64_t* out_tri, float* out_vw,
                                   hipStream_t s);
hipError_t launch_mesh_count_hits(const miso_mesh_plan_t& plan, const void* workspace, const int32_t* lists, int64_t capacity,
                                  const float* org, int64_t ld_o, const float* dir, int64_t ld_d, int64_t n, float t_min, float t_max,
                                  int32_t* out_count, hipStream_t s);
hipError_t launch_mesh_count_hits_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t,
                                      int64_t n_tri, const float* org, int64_t ld_o, const float* dir, int64_t ld_d, int64_t n,
                                      float t_min, float t_max, int32_t* out_count, hipStream_t s);

}  // namespace miso
