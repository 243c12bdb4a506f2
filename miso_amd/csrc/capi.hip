// extern "C" entry points of libmiso_hip.so (see include/miso_hip.h): each one is the named argument checks of its
// family (the anonymous namespace below), the conversion to the kernel-side structs, then the launch -- nothing is
// launched before every check has passed.  tests/golden/capi_refusals.json pins every refusal.
//
// Sibling differences, kept as found (a behaviour fix is its own change; the refusal table records each):
//  * a count >= 2^31 is MISO_E_BADARG from miso_nn_knn, miso_nn_knn_all_pairs, miso_nn_knn_normals, miso_sort_points and
//    miso_atlas_sdf_fwd's lattice; MISO_E_TOOLARGE from every other entry point.
//  * mlp == NULL is MISO_E_BADARG from miso_sdf_bwd_rows, miso_sdf_wgrad and the three atlas calls; MISO_E_UNSUPPORTED
//    from the other fused calls (and from miso_mlp_pack, which says UNSUPPORTED for packed == NULL too).
//  * a loss type out of range is MISO_E_BADARG from the mapping-loss and alignment calls, MISO_E_UNSUPPORTED from
//    miso_lm_normal_eq, miso_lm_track_step and miso_track_adam_step.
//  * n == 0: miso_sdf_fwd_loss zeroes the loss slots without looking at grid, mlp or packed (at `sorted` it does look),
//    miso_sdf_train checks them first; miso_atlas_sdf_bwd and miso_atlas_sphere_trace return before their per-point
//    pointers are looked at, miso_atlas_sdf_fwd has no such return.
//  * the tracker steps check grid shape, mlp and packed in the fused forward, BEHIND their first launch (the head).
//  * miso_sdf_bwd_rows refuses the host-side gradient flags (OVERWRITE, SDF_SORTED, ZEROED); of a caller-order batch
//    miso_sdf_bwd refuses SDF_SORTED and ignores the other two -- and so do its callers here: miso_sdf_bwd_rows without
//    rows, and miso_lm_track_step and miso_track_adam_step (behind their first launch, like their other grid checks).
//  * miso_adam_dense asks no alignment of its four arrays; miso_adam_step asks 16 bytes of them, and 4 bytes of the
//    flag arrays where `touched` is given (even for numel == 0).
#include <stdlib.h>
#include <string.h>

#include "common.hpp"
#include "align.hpp"
#include "checks.hpp"
#include "grad_plan.hpp"
#include "launch.hpp"
#include "version.inc"

using namespace miso;

namespace {

// ---- small predicates --------------------------------------------------------------------------------------------------
inline bool fits32(int64_t n) { return n < ((int64_t)1 << 31); }            // a size the 32-bit index math holds
inline bool fits_fp32_count(int64_t n) { return n < ((int64_t)1 << 24); }   // ... an fp32 counter holds exactly
inline bool fits_voxel_key(int64_t n) { return n < ((int64_t)1 << 22); }    // ... the index field of the voxel sort key holds
// (aligned, all_set, set_if: checks.hpp)
inline bool mapping_loss_ok(int loss_type) { return loss_type == 1 || loss_type == 2; }                  // L1 | L2

int convert_grid(const miso_grid_t* in, GridK* out, bool need_data, bool* vec4) {
  if (!in || in->n_levels < 1 || in->n_levels > MISO_MAX_LEVELS) return MISO_E_BADARG;
  if (in->flags & ~(MISO_F_ALIGN_CORNERS | MISO_F_PAD_BORDER | MISO_F_COORDS_NORMALIZED | MISO_F_GRAD_OVERWRITE |
                    MISO_F_GRAD_SDF_SORTED | MISO_F_GRAD_ZEROED | MISO_F_CROWDED | MISO_F_EXACT_F32 | MISO_F_FULL_TRIPS))
    return MISO_E_BADARG;
  memset(out, 0, sizeof(*out));
  out->n_levels = in->n_levels;
  out->ignore_mask = in->ignore_mask;
  out->flags = in->flags & ~(MISO_F_GRAD_OVERWRITE | MISO_F_GRAD_SDF_SORTED | MISO_F_GRAD_ZEROED);   // host-side flags
  for (int a = 0; a < 3; ++a) { out->bmin[a] = in->bound_min[a]; out->bmax[a] = in->bound_max[a]; out->gscale[a] = 1.0f; }
  out->xstride = 3;
  bool v4 = true;
  int foff = 0;
  for (int l = 0; l < in->n_levels; ++l) {
    const miso_level_t& s = in->level[l];
    if (s.C < 1 || s.X < 1 || s.Y < 1 || s.Z < 1) return MISO_E_BADARG;
    if (need_data && !s.data) return MISO_E_BADARG;
    if (s.sC < 0 || s.sX < 0 || s.sY < 0 || s.sZ < 0) return MISO_E_BADARG;
    if (!fits32(level_span(s))) return MISO_E_TOOLARGE;
    LevelK& d = out->lv[l];
    d.data = s.data; d.grad = s.grad; d.gg = nullptr;
    d.touched = s.grad ? s.grad_touched : nullptr;
    d.C = s.C; d.X = s.X; d.Y = s.Y; d.Z = s.Z;
    d.sC = (int32_t)s.sC; d.sX = (int32_t)s.sX; d.sY = (int32_t)s.sY; d.sZ = (int32_t)s.sZ;
    d.foff = foff;
    foff += s.C;
    bool ok = (s.C % 4 == 0) && (s.sC == 1 || s.C == 1) && (s.sX % 4 == 0) && (s.sY % 4 == 0) &&
              (s.sZ % 4 == 0) && aligned(16, s.data, s.grad);
    v4 = v4 && ok;
  }
  out->F = foff;
  if (vec4) *vec4 = v4;
  return MISO_OK;
}

int fused_shape(const GridK& g, bool vec4, const miso_mlp_t* m, int* C, int* L, int* H, int* NH) {
  if (!m || !vec4) return MISO_E_UNSUPPORTED;
  if (m->n_linear < 2 || m->n_linear > MISO_MAX_LINEAR) return MISO_E_UNSUPPORTED;
  int c = g.lv[0].C;
  for (int l = 0; l < g.n_levels; ++l)
    if (g.lv[l].C != c) return MISO_E_UNSUPPORTED;
  if (m->in_dim != g.F || m->out_dim != 1) return MISO_E_UNSUPPORTED;
  int nh = m->n_linear - 2;
  if (!fused_shape_supported(c, g.n_levels, m->hidden_dim, nh)) return MISO_E_UNSUPPORTED;
  *C = c; *L = g.n_levels; *H = m->hidden_dim; *NH = nh;
  return MISO_OK;
}

// ---- the fused call: grid + decoder as the fused kernels take them ----------------------------------------------------
struct FusedCall { GridK g; bool vec4; int C, L, H, NH; };      // (C, L, H, NH): the kernel table's key
// FUSED_ATLAS: `grid` is the atlas' shape grid -- the levels the kernels address are the plan's, which
// miso_atlas_plan_build admitted as 16-byte addressable, so the shape's own vec4 is not asked; the key starts from the
// one decoder the atlas kernels were first built for (H = 64, NH = 1)
enum FusedKind { FUSED_GRID, FUSED_ATLAS };

// the grid half: what a query for features only stops at (miso_atlas_sdf_fwd without sdf)
int fused_grid(FusedCall* f, const miso_grid_t* grid, bool need_data) {
  if (int rc = convert_grid(grid, &f->g, need_data, &f->vec4)) return rc;
  f->C = f->g.lv[0].C; f->L = f->g.n_levels; f->H = 64; f->NH = 1;
  return MISO_OK;
}
// the queries' form: no packed weights
int fused_query(FusedCall* f, const miso_grid_t* grid, const miso_mlp_t* mlp, bool need_data, FusedKind kind = FUSED_GRID) {
  if (int rc = fused_grid(f, grid, need_data)) return rc;
  return fused_shape(f->g, kind == FUSED_ATLAS ? true : f->vec4, mlp, &f->C, &f->L, &f->H, &f->NH);
}
// the launching form: `packed` (miso_mlp_pack's output) is read with 16-byte loads
int fused_call(FusedCall* f, const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, bool need_data,
               FusedKind kind = FUSED_GRID) {
  if (!packed || !aligned(16, packed)) return MISO_E_BADARG;
  return fused_query(f, grid, mlp, need_data, kind);
}

// ---- the atlas call: plan, pose table and flags of the three atlas entry points -----------------------------------------
int atlas_call(AtlasK* a, const void* plan, int32_t n_submaps, const float* poses, int64_t n, uint32_t flags) {
  if (!plan || !poses || n_submaps < 1 || n < 0) return MISO_E_BADARG;
  if (flags & ~(MISO_F_EXACT_F32 | MISO_F_ATLAS_NO_BOUND)) return MISO_E_BADARG;
  memset(a, 0, sizeof(*a));
  a->submaps = reinterpret_cast<const GridK*>(plan);
  a->poses = poses; a->n_submaps = n_submaps; a->n = n;
  a->no_bound = (flags & MISO_F_ATLAS_NO_BOUND) ? 1 : 0;
  return MISO_OK;
}

// ---- clouds, ray pairs, the caller's mesh arrays, an index with its workspace ----------------------------------------------
// a cloud p (n, 3) of row pitch ld, and what the call writes per point
template <class... Out> int check_cloud(const float* p, int64_t ld, int64_t n, const Out*... out) {
  if (ld < 3 || n < 0) return MISO_E_BADARG;
  if (!fits32(n)) return MISO_E_TOOLARGE;
  return set_if(n, p, out...) ? MISO_OK : MISO_E_BADARG;
}
// kept as found: the k-nearest calls say BADARG where their siblings say TOOLARGE
inline int knn_code(int rc) { return rc == MISO_E_TOOLARGE ? MISO_E_BADARG : rc; }

// n rays: origins and dirs (n, 3) of their row pitches, and what the call writes per ray
template <class... Out> int check_rays(const float* origins, int64_t ld_o, const float* dirs, int64_t ld_d, int64_t n,
                                       const Out*... out) {
  if (ld_o < 3 || ld_d < 3 || n < 0) return MISO_E_BADARG;
  if (!fits32(n)) return MISO_E_TOOLARGE;
  return set_if(n, origins, dirs, out...) ? MISO_OK : MISO_E_BADARG;
}

// a mesh in the caller's arrays: verts (n_vert, 3) fp32, tris (n_tri, 3) int64 (a mesh of triangles without a vertex is
// one whose triangles are never hit)
int check_mesh_arrays(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t, int64_t n_tri) {
  if (n_vert < 0 || n_tri < 0 || ld_v < 3 || ld_t < 3) return MISO_E_BADARG;
  if (!fits32(n_tri)) return MISO_E_TOOLARGE;
  return n_tri == 0 || (tris && (n_vert == 0 || verts)) ? MISO_OK : MISO_E_BADARG;
}

// an index over `indexed` targets or triangles has them in its workspace, which the kernels read with 16-byte loads
inline bool index_ready(int64_t indexed, const void* workspace) {
  return indexed == 0 || (workspace && aligned(16, workspace));
}

// the cell grid of a plan, as miso_nn_plan writes it for both kinds of index (MISO_MESH_MAX_CELLS == MISO_NN_MAX_CELLS)
bool plan_grid_ok(const int32_t dims[3], int64_t cells, float cell, float coord_mag) {
  if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || cells < 1 || cells > MISO_NN_MAX_CELLS) return false;
  if ((int64_t)dims[0] * dims[1] > MISO_NN_MAX_CELLS || (int64_t)dims[0] * dims[1] * dims[2] != cells) return false;
  return cell > 0.0f && cell < __builtin_huge_valf() && coord_mag >= 0.0f;
}
// a plan as miso_nn_plan / miso_mesh_plan writes it (the struct is the caller's memory: the kernels index by it)
bool nn_plan_ok(const miso_nn_plan_t* p) {
  if (!p || p->n_tgt < 0 || !fits32(p->n_tgt) || p->max_rings < 0 || p->max_rings > MISO_NN_MAX_RINGS) return false;
  return plan_grid_ok(p->dims, p->cells, p->cell, p->coord_mag);
}
bool mesh_plan_ok(const miso_mesh_plan_t* p) {
  if (!p || p->n_tri < 0 || !fits32(p->n_tri)) return false;
  return plan_grid_ok(p->dims, p->cells, p->cell, p->coord_mag) && p->coord_mag < __builtin_huge_valf() &&
         p->widen >= 0.0f && p->widen <= p->coord_mag;
}
// a mesh index as miso_mesh_build fills it, or left it: plan, workspace and the per-cell lists
bool mesh_index_ok(const miso_mesh_plan_t* p, const void* workspace, const int32_t* lists, int64_t capacity) {
  if (!mesh_plan_ok(p) || capacity < 0) return false;
  return p->n_tri == 0 || (index_ready(p->n_tri, workspace) && (capacity == 0 || lists));
}
inline bool nn_k_ok(int32_t k) { return k >= 1 && k <= MISO_NN_KNN_MAX; }

// ---- Adam: the pointers of one tensor --------------------------------------------------------------------------------------
// the four arrays are read and written 16 bytes at a time; the flag bytes four at a time where `touched` drives the step
bool adam_tensor_ok(const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                    const uint8_t* active, const uint8_t* touched, int64_t numel) {
  if (numel < 0 || !set_if(numel, param, grad, exp_avg, exp_avg_sq, active)) return false;
  if (!aligned(16, param, grad, exp_avg, exp_avg_sq)) return false;
  return !touched || aligned(4, active, touched);
}
bool adam_tensors_ok(const miso_adam_tensor_t* tensors, int32_t n_tensors) {
  if (!tensors || n_tensors < 1 || n_tensors > MISO_ADAM_MAX_TENSORS) return false;
  for (int i = 0; i < n_tensors; ++i) {
    const miso_adam_tensor_t& t = tensors[i];
    if (!adam_tensor_ok(t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.active, t.touched, t.numel)) return false;
  }
  return true;
}

// ---- tracker: miso_lm_track_t as both steps read it -------------------------------------------------------------------------
// step_scratch: the one per-row buffer that differs between the steps (ones | grad_pred)
bool lm_track_ok(const miso_lm_track_t* a, const float* step_scratch) {
  if (a->n < 0 || !all_set(a->R_base, a->t_base, a->rot_correction, a->trans_correction, a->pose, a->sums, a->info)) return false;
  if (!set_if(a->n, a->coords_frame, a->target, a->coords_world, a->sdf, a->grad, a->relu_mask, step_scratch)) return false;
  return a->stride_target >= 0 && a->stride_valid >= 0 && a->stride_frame_ids >= 0;
}
// the steps want d sdf / d x only: a grid that carries a gradient buffer is refused
bool has_grad_buffers(const miso_grid_t* grid) {
  for (int l = 0; l < grid->n_levels && l < MISO_MAX_LEVELS; ++l)
    if (grid->level[l].grad) return true;
  return false;
}

// what a call asks of plan_grad (sorted == nullptr: an unbinned batch, nothing is pulled), the pointers its launch reads
GradAsk grad_ask(GradCaller who, bool v4, const miso_grid_t* grid, const miso_sorted_t* sorted, int64_t n, int64_t ld,
                 const void* workspace, bool ggx) {
  GradAsk a = {who, v4, grid->flags, n, ld, ggx, workspace && aligned(16, workspace), false, false, 0, 0};
  if (!sorted) return a;
  a.sorted = true; a.xn = sorted->xn_sorted != nullptr; a.tiles = sorted->tiles_per_axis;
  a.queue_ints = sorted->pull_queue ? sorted->pull_queue_ints : 0;
  return a;
}
PullBatch pull_batch(const miso_sorted_t* s, const float* dfeat, const int* perm, const float* ggx) {
  return PullBatch{s->tile_offsets, s->xn_sorted, dfeat, perm, ggx, s->pull_queue};
}

// the loss side of a fused launch: the mapping loss's parameters, its input rows, where d loss / d sdf (binned order) and
// the loss slots go; the mean is over n rows, or over *n_live of a padded batch
LossInK loss_in(int loss_type, float w_sdf, float w_fs, float trunc, const float* loss_inputs, float* gsdf_sorted,
                float* loss_slots, int64_t n, const int32_t* n_live) {
  LossInK lin;
  memset(&lin, 0, sizeof(lin));
  lin.p.loss_type = loss_type; lin.p.w_sdf = w_sdf; lin.p.w_fs = w_fs; lin.p.trunc = trunc;
  lin.aux = reinterpret_cast<const float4*>(loss_inputs);
  lin.gsdf_sorted = gsdf_sorted; lin.loss_out = loss_slots;
  lin.inv_n = 1.0f / (float)n;
  lin.n_live = n_live;
  return lin;
}
// an empty batch has a loss of zero: every slot is written, as by a launch
hipError_t zero_loss_slots(float* loss_slots, hipStream_t stream) {
  return launch_zero_words(loss_slots, MISO_LOSS_SLOTS * 2, stream);
}

// perm_optional: the entry point can take the original index from xn_sorted[p].w (miso_sdf_train)
int check_sorted(const miso_sorted_t* s, int64_t n, bool perm_optional = false) {
  if (!s || !s->tile_offsets) return MISO_E_BADARG;
  if (n > 0 && (!s->x_sorted && !s->xn_sorted)) return MISO_E_BADARG;   // an empty batch has no buffers
  if (n > 0 && !s->perm && !(perm_optional && s->xn_sorted)) return MISO_E_BADARG;
  if (!aligned(16, s->xn_sorted)) return MISO_E_BADARG;
  { int t3_[3]; if (!tiles_xyz(s->tiles_per_axis, t3_)) return MISO_E_BADARG; }
  return MISO_OK;
}

// Sorted batches: read the pre-normalised float4 points instead of the metric ones.
const float* sorted_points(GridK* g, const miso_sorted_t* sorted) {
  if (!sorted->xn_sorted) return sorted->x_sorted;
  if (!(g->flags & MISO_F_COORDS_NORMALIZED)) {
    for (int a = 0; a < 3; ++a) g->gscale[a] = 2.0f / (g->bmax[a] - g->bmin[a]);   // axis_coord's m
    g->flags |= MISO_F_COORDS_NORMALIZED;
  }
  g->xstride = 4;
  return sorted->xn_sorted;
}

// The points of a call, by the one rule of miso_hip.h (at miso_sorted_t).  sorted != NULL, the binned form: `sorted` is
// checked, *x and *perm are taken from it and g reads the points it has (the caller's x is ignored).  sorted == NULL,
// the caller's order: *x as given, which n > 0 points need, and no perm.
int use_points(GridK* g, const float** x, const int** perm, const miso_sorted_t* sorted, int64_t n,
               bool perm_optional = false) {
  *perm = nullptr;
  if (sorted) {
    if (int rc = check_sorted(sorted, n, perm_optional)) return rc;
    *x = sorted_points(g, sorted);
    *perm = sorted->perm;
  }
  return n > 0 && !*x ? MISO_E_BADARG : MISO_OK;
}

int mc_check_dims(int32_t nx, int32_t ny, int32_t nz) {
  if (nx < 1 || ny < 1 || nz < 1) return MISO_E_BADARG;
  // cell ids are 32-bit; sample indices (and keys = 3 * index + axis) are 64-bit
  if (!fits32((int64_t)nx * ny * nz)) return MISO_E_TOOLARGE;
  return 0;
}

}  // namespace

extern "C" {

const char* miso_version(void) { return "miso_hip 0.2 (gfx950) src=" MISO_SOURCE_HASH; }

const char* miso_error_string(int code) {
  switch (code) {
    case MISO_OK: return "ok";
    case MISO_E_BADARG: return "bad argument";
    case MISO_E_UNSUPPORTED: return "shape not covered by the fused kernels";
    case MISO_E_TOOLARGE: return "a grid level spans >= 2^31 elements";
    default: return hipGetErrorString((hipError_t)code);
  }
}

int miso_encode_fwd(const miso_grid_t* grid, const float* x, const miso_sorted_t* sorted, int64_t n, float* feats,
                    int64_t ld_out, void* stream) {
  if (n < 0 || !set_if(n, feats)) return MISO_E_BADARG;
  GridK g; bool v4;
  if (int rc = convert_grid(grid, &g, true, &v4)) return rc;
  if (ld_out < g.F) return MISO_E_BADARG;
  const int* perm;
  if (int rc = use_points(&g, &x, &perm, sorted, n)) return rc;
  return (int)launch_encode_fwd(g, v4, x, n, feats, ld_out, perm, (hipStream_t)stream);
}

int miso_encode_bwd(const miso_grid_t* grid, const float* x, const miso_sorted_t* sorted, int64_t n,
                    const float* grad_feats, int64_t ld_g, float* grad_x, void* stream) {
  if (n < 0 || !set_if(n, grad_feats)) return MISO_E_BADARG;
  GridK g; bool v4;
  if (int rc = convert_grid(grid, &g, grad_x != nullptr, &v4)) return rc;
  if (ld_g < g.F) return MISO_E_BADARG;
  const int* perm;
  if (int rc = use_points(&g, &x, &perm, sorted, n)) return rc;
  return (int)launch_encode_bwd(g, v4, x, n, grad_feats, ld_g, grad_x, perm, (hipStream_t)stream);
}

int miso_encode_bwd2(const miso_grid_t* grid, const miso_grid_t* gg_grid, const float* x, const miso_sorted_t* sorted,
                     int64_t n, const float* grad_feats, int64_t ld_g, const float* gg_x, float* gg_out,
                     int64_t ld_gg, float* g_x, void* stream) {
  if (n < 0 || !set_if(n, grad_feats, gg_out)) return MISO_E_BADARG;
  GridK g; bool v4;
  if (int rc = convert_grid(grid, &g, true, &v4)) return rc;
  if (ld_g < g.F || ld_gg < g.F) return MISO_E_BADARG;
  if (gg_grid) {
    if (gg_grid->n_levels != grid->n_levels) return MISO_E_BADARG;
    for (int l = 0; l < g.n_levels; ++l) {
      const miso_level_t& a = grid->level[l];
      const miso_level_t& b = gg_grid->level[l];
      if (!b.data) continue;
      if (a.C != b.C || a.X != b.X || a.Y != b.Y || a.Z != b.Z || a.sC != b.sC || a.sX != b.sX ||
          a.sY != b.sY || a.sZ != b.sZ)
        return MISO_E_BADARG;  // cotangent must share the layout of the grid
      if (!aligned(16, b.data)) v4 = false;
      g.lv[l].gg = b.data;
    }
  }
  const int* perm;
  if (int rc = use_points(&g, &x, &perm, sorted, n)) return rc;
  return (int)launch_encode_bwd2(g, v4, x, n, grad_feats, ld_g, gg_x, gg_out, ld_gg, g_x, perm,
                                 (hipStream_t)stream);
}

int64_t miso_mlp_packed_floats(const miso_mlp_t* mlp) {
  if (!mlp || mlp->n_linear < 2 || mlp->n_linear > MISO_MAX_LINEAR) return 0;
  if (mlp->out_dim != 1 || mlp->in_dim < 1 || mlp->in_dim > 32) return 0;
  if (mlp->hidden_dim != 32 && mlp->hidden_dim != 64) return 0;
  return mlp_packed_floats(mlp->in_dim, mlp->hidden_dim, mlp->n_linear - 2);
}

int64_t miso_sdf_mask_words(const miso_mlp_t* mlp) {
  if (!mlp) return 0;
  return (int64_t)(mlp->n_linear - 1) * (mlp->hidden_dim / 32);
}

int miso_mlp_pack(const miso_mlp_t* mlp, float* packed, void* stream) {
  if (!packed || miso_mlp_packed_floats(mlp) == 0) return MISO_E_UNSUPPORTED;
  MlpK k;
  memset(&k, 0, sizeof(k));
  for (int i = 0; i < mlp->n_linear; ++i) {
    if (!mlp->weight[i]) return MISO_E_BADARG;
    k.w[i] = mlp->weight[i];
    k.b[i] = mlp->bias[i];
  }
  return (int)launch_mlp_pack(k, mlp->in_dim, mlp->hidden_dim, mlp->n_linear - 2, packed,
                              (hipStream_t)stream);
}

int64_t miso_sdf_train_lds_bytes(const miso_grid_t* grid, const miso_mlp_t* mlp, int32_t scattering) {
  FusedCall f;
  if (fused_query(&f, grid, mlp, false)) return 0;
  return sdf_train_lds_bytes(f.C, f.L, f.H, f.NH, scattering != 0);
}

int miso_sdf_supported(const miso_grid_t* grid, const miso_mlp_t* mlp) {
  FusedCall f;
  return fused_query(&f, grid, mlp, false) == MISO_OK ? 1 : 0;
}

// the forward of miso_sdf_fwd and, with `loss`, of miso_sdf_fwd_loss
static int sdf_fwd(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const float* x,
                   const miso_sorted_t* sorted, int64_t n, float* sdf, uint32_t* relu_mask, void* stream,
                   const LossInK* loss) {
  LossInK lin;
  memset(&lin, 0, sizeof(lin));
  if (loss) lin = *loss;
  if (n < 0 || (n > 0 && !sdf && !loss)) return MISO_E_BADARG;
  FusedCall f;
  if (int rc = fused_call(&f, grid, mlp, packed, true)) return rc;
  const int* perm;
  if (int rc = use_points(&f.g, &x, &perm, sorted, n)) return rc;
  return (int)launch_sdf_fwd(f.C, f.L, f.H, f.NH, f.g, packed, x, n, sdf, relu_mask, perm, lin, (hipStream_t)stream);
}

int miso_sdf_fwd(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const float* x,
                 const miso_sorted_t* sorted, int64_t n, float* sdf, uint32_t* relu_mask, void* stream) {
  return sdf_fwd(grid, mlp, packed, x, sorted, n, sdf, relu_mask, stream, nullptr);
}

int miso_sdf_fwd_loss(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const float* x,
                      const miso_sorted_t* sorted, int64_t n, int loss_type, float weight_sdf, float weight_fs,
                      float trunc_dist, const float* loss_inputs, float* sdf, uint32_t* relu_mask, float* grad_sdf,
                      float* loss_slots, const int32_t* n_live, void* stream) {
  if (!mapping_loss_ok(loss_type) || !loss_slots || n < 0 || !set_if(n, loss_inputs, grad_sdf) || !aligned(16, loss_inputs))
    return MISO_E_BADARG;
  if (!sorted && n_live) return MISO_E_BADARG;      // a padded batch is a binned one
  if (n == 0) {                                     // kept as found: of an empty batch only `sorted` is looked at
    if (int rc = sorted ? check_sorted(sorted, n) : MISO_OK) return rc;
    return (int)zero_loss_slots(loss_slots, (hipStream_t)stream);
  }
  const LossInK lin = loss_in(loss_type, weight_sdf, weight_fs, trunc_dist, loss_inputs, grad_sdf, loss_slots, n, n_live);
  return sdf_fwd(grid, mlp, packed, x, sorted, n, sdf, relu_mask, stream, &lin);
}

int miso_sdf_bwd(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const float* x,
                 const miso_sorted_t* sorted, int64_t n, const float* grad_sdf, const uint32_t* relu_mask,
                 float* grad_x, float* workspace, void* stream) {
  if (n < 0 || !set_if(n, grad_sdf, relu_mask)) return MISO_E_BADARG;
  FusedCall f;
  if (int rc = fused_call(&f, grid, mlp, packed, grad_x != nullptr)) return rc;
  const bool gsdf_sorted = (grid->flags & MISO_F_GRAD_SDF_SORTED) != 0;
  if (!sorted && (workspace || gsdf_sorted)) return MISO_E_BADARG;      // the binned form's
  const GridK& g = f.g;
  GridK gp = g;                                   // sample positions as the kernels read them
  const int* perm;
  if (int rc = use_points(&gp, &x, &perm, sorted, n)) return rc;
  // owned levels leave their d-feat rows in the workspace (a pushed level's go the same way); the rest is scattered
  const GradPlan plan = plan_grad(g, grad_ask(GRAD_BWD, f.vec4, grid, sorted, n, g.F, workspace, false), pull_knobs());
  const bool want_grid = plan.want != 0;
  if (!want_grid && !grad_x) return MISO_OK;
  if (plan.refuse) return MISO_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = zero_level_grads(g, plan.fill, st);
  if (e != hipSuccess) return (int)e;
  if (n == 0 && !plan.owned) return MISO_OK;
  if (n > 0) {
    e = launch_sdf_bwd(f.C, f.L, f.H, f.NH, gp, packed, x, n, grad_sdf, relu_mask, grad_x, want_grid, perm,
                       plan.owned ? workspace : nullptr, plan.owned, gsdf_sorted, st);
    if (e != hipSuccess) return (int)e;
  }
  if (!plan.owned) return MISO_OK;
  return (int)launch_grad_pull(g, plan, pull_batch(sorted, workspace, nullptr, nullptr), st);
}

// The first backward with its d-feat rows handed out: what the SECOND backward (create_graph=True: eikonal / smoothness
// terms, loss_isdf.py:96-152,367-377) differentiates -- d sdf / d x = J_E(x; G)^T rows, and the decoder, piecewise linear,
// contributes nothing else (miso_encode_bwd2 on these rows is the whole double backward).
int miso_sdf_bwd_rows(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const float* x, int64_t n,
                      const float* grad_sdf, const uint32_t* relu_mask, float* grad_x, float* dfeat_rows, void* stream) {
  if (!grid || !mlp) return MISO_E_BADARG;
  if (!dfeat_rows) return miso_sdf_bwd(grid, mlp, packed, x, nullptr, n, grad_sdf, relu_mask, grad_x, nullptr, stream);
  if (n < 0 || !set_if(n, grad_sdf, relu_mask, x) || !aligned(16, dfeat_rows)) return MISO_E_BADARG;
  if (grid->flags & (MISO_F_GRAD_OVERWRITE | MISO_F_GRAD_SDF_SORTED | MISO_F_GRAD_ZEROED)) return MISO_E_BADARG;
  FusedCall f;
  if (int rc = fused_call(&f, grid, mlp, packed, grad_x != nullptr)) return rc;
  if (n == 0) return MISO_OK;
  // want_grid = true selects the kernel form that stages the d-feat tile; levels without a gradient buffer are not scattered
  return (int)launch_sdf_bwd(f.C, f.L, f.H, f.NH, f.g, packed, x, n, grad_sdf, relu_mask, grad_x, true, nullptr, dfeat_rows, 0u,
                             false, (hipStream_t)stream);
}

int64_t miso_sort_workspace_bytes(int64_t n, int32_t tiles_per_axis) {
  if (n < 0) return 0;
  return sort_workspace_bytes(n, tiles_per_axis);
}

int miso_sort_points(const miso_grid_t* grid, const float* x, int64_t n, int32_t tiles_per_axis,
                     void* workspace, float* x_sorted, float* xn_sorted, int32_t* perm,
                     int32_t* tile_offsets, void* stream) {
  { int t3_[3]; if (n < 0 || !fits32(n) || !tiles_xyz(tiles_per_axis, t3_)) return MISO_E_BADARG; }
  if (!workspace || !tile_offsets || (n > 0 && (!x || (!x_sorted && !xn_sorted)))) return MISO_E_BADARG;
  if (n > 0 && !perm && !xn_sorted) return MISO_E_BADARG;      // without perm the index lives in xn_sorted[p].w only
  if (!aligned(16, xn_sorted)) return MISO_E_BADARG;
  GridK g;
  if (int rc = convert_grid(grid, &g, false, nullptr)) return rc;
  return (int)launch_sort(g, x, n, tiles_per_axis, workspace, x_sorted, xn_sorted, perm, tile_offsets,
                          (hipStream_t)stream);
}

// The plan a binned backward or training step of n samples follows with every buffer in place: what the four queries
// report.  All zero (nothing owned, PULL_NONE) for a grid or a tiles code the entry points refuse.
static GradPlan query_plan(const miso_grid_t* grid, int32_t tiles, int64_t n, int64_t ld) {
  GridK g; bool v4;
  if (convert_grid(grid, &g, false, &v4)) return GradPlan{};
  GradAsk a = grad_ask(GRAD_BWD, v4, grid, nullptr, n, ld, nullptr, false);
  a.tiles = tiles; a.sorted = a.xn = a.workspace = true;
  const GradPlan p = plan_grad(g, a, pull_knobs());
  return p.valid ? p : GradPlan{};
}

uint32_t miso_sdf_bwd_scattered_levels(const miso_grid_t* grid, int32_t tiles_per_axis, int64_t n) {
  const GradPlan p = query_plan(grid, tiles_per_axis, n, 0);
  return p.scatter | p.push;      // every level that atomics add to
}
uint32_t miso_sdf_bwd_push_levels(const miso_grid_t* grid, int32_t tiles_per_axis, int64_t n) {
  return query_plan(grid, tiles_per_axis, n, 0).push;
}
int miso_grad_pull_on_matrix_cores(const miso_grid_t* grid, int32_t tiles_per_axis, int64_t n, int64_t ld_d) {
  return query_plan(grid, tiles_per_axis, n, ld_d).form == PULL_MC ? 1 : 0;
}
uint32_t miso_grad_pull_levels(const miso_grid_t* grid, int32_t tiles_per_axis) {
  return query_plan(grid, tiles_per_axis, 0, 0).owned;
}

static int grad_pull_impl(const miso_grid_t* grid, const miso_sorted_t* sorted, int64_t n, const float* dfeat,
                          int64_t ld_d, int32_t rows_in_caller_order, const float* gg_x, void* stream) {
  if (int rc = check_sorted(sorted, n)) return rc;
  if (n < 0 || !set_if(n, sorted->xn_sorted, dfeat) || !aligned(16, dfeat) || (ld_d & 3) != 0) return MISO_E_BADARG;
  GridK g; bool v4;
  if (int rc = convert_grid(grid, &g, false, &v4)) return rc;
  if (ld_d < g.F) return MISO_E_BADARG;
  const GradPlan plan = plan_grad(g, grad_ask(GRAD_PULL, v4, grid, sorted, n, ld_d, dfeat, gg_x != nullptr), pull_knobs());
  if (plan.refuse) return MISO_E_UNSUPPORTED;
  if (gg_x && !(g.flags & MISO_F_COORDS_NORMALIZED))
    for (int a = 0; a < 3; ++a) g.gscale[a] = 2.0f / (g.bmax[a] - g.bmin[a]);   // d xn / d x (axis_coord's m)
  return (int)launch_grad_pull(g, plan, pull_batch(sorted, dfeat, rows_in_caller_order ? sorted->perm : nullptr, gg_x),
                               (hipStream_t)stream);
}

int miso_grad_pull(const miso_grid_t* grid, const miso_sorted_t* sorted, int64_t n, const float* dfeat,
                   int64_t ld_d, int32_t rows_in_caller_order, void* stream) {
  return grad_pull_impl(grid, sorted, n, dfeat, ld_d, rows_in_caller_order, nullptr, stream);
}

int miso_grad_pull_dx(const miso_grid_t* grid, const miso_sorted_t* sorted, int64_t n, const float* grad_feats,
                      int64_t ld_g, const float* gg_x, void* stream) {
  if (!gg_x) return MISO_E_BADARG;
  return grad_pull_impl(grid, sorted, n, grad_feats, ld_g, 1, gg_x, stream);
}

int64_t miso_sdf_bwd_workspace_floats(const miso_grid_t* grid, int64_t n) {
  GridK g;
  if (n < 0 || convert_grid(grid, &g, false, nullptr)) return 0;
  return n * g.F;
}

int64_t miso_sdf_wgrad_workspace_floats(const miso_grid_t* grid, const miso_mlp_t* mlp, int64_t n) {
  FusedCall f;
  if (n < 0 || fused_query(&f, grid, mlp, false)) return 0;
  return sdf_wgrad_workspace_floats(f.C, f.L, f.H, f.NH, n);
}

// The decoder's weight and bias gradients (decoder_wgrad.hip): the sign bits and the point order are those of the forward
// that wrote relu_mask (miso_sdf_fwd over the same x / sorted).
int miso_sdf_wgrad(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const float* x, int64_t n,
                   const float* grad_sdf, const uint32_t* relu_mask, const miso_sorted_t* sorted, uint32_t flags,
                   const miso_mlp_grad_t* grads, float* workspace, int64_t workspace_floats, void* stream) {
  if (!grid || !mlp || !grads || n < 0 || !set_if(n, grad_sdf, relu_mask)) return MISO_E_BADARG;
  if ((flags & ~MISO_F_GRAD_SDF_SORTED) || ((flags & MISO_F_GRAD_SDF_SORTED) && !sorted)) return MISO_E_BADARG;
  FusedCall f;
  if (int rc = fused_call(&f, grid, mlp, packed, n > 0)) return rc;
  WgradOutK out;
  memset(&out, 0, sizeof(out));
  for (int l = 0; l < mlp->n_linear; ++l) {
    if (!grads->weight[l]) return MISO_E_BADARG;
    out.w[l] = grads->weight[l];
    out.b[l] = grads->bias[l];
  }
  const int64_t need = sdf_wgrad_workspace_floats(f.C, f.L, f.H, f.NH, n);
  if (need > 0 && (!workspace || workspace_floats < need || !aligned(16, workspace))) return MISO_E_BADARG;
  const int* perm;
  if (int rc = use_points(&f.g, &x, &perm, sorted, n)) return rc;
  return (int)launch_sdf_wgrad(f.C, f.L, f.H, f.NH, f.g, packed, x, n, grad_sdf, relu_mask, perm,
                               (flags & MISO_F_GRAD_SDF_SORTED) != 0, out, workspace, (hipStream_t)stream);
}

// One training iteration of a frozen-decoder submap: forward + mapping loss + decoder backward in ONE launch
// (sdf_train_kernel).  sorted != nullptr: a binned batch -- the levels the pull / push can form get their gradient from
// the d-feat rows left in `workspace`, the others (bricks beyond the pull's reach) are scattered with float atomics from
// the kernel itself.  sorted == nullptr: an unbinned batch (x in the caller's order), every level scattered.
int miso_sdf_train(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const float* x,
                   const miso_sorted_t* sorted, int64_t n, int loss_type, float weight_sdf, float weight_fs,
                   float trunc_dist, const float* loss_inputs, float* sdf, float* loss_slots, const int32_t* n_live,
                   float* workspace, void* stream) {
  if (!mapping_loss_ok(loss_type) || !loss_slots || n < 0 || !set_if(n, loss_inputs)) return MISO_E_BADARG;
  if (!aligned(16, loss_inputs, workspace)) return MISO_E_BADARG;
  // the binned step leaves d-feat rows in the workspace and reads the float4 points; the other form has neither
  if (sorted ? n > 0 && (!workspace || !sorted->xn_sorted) : n_live || workspace) return MISO_E_BADARG;
  FusedCall f;
  if (int rc = fused_call(&f, grid, mlp, packed, true)) return rc;
  const GridK& g = f.g;
  GridK gp = g;                                   // sample positions as the kernel reads them
  const int* perm;
  if (int rc = use_points(&gp, &x, &perm, sorted, n, true)) return rc;
  if (sorted && !perm) gp.flags |= MISO_F_INDEX_IN_XN;
  // owned levels are formed from the d-feat rows (pull or push); the rest is scattered from the kernel
  const GradPlan plan = plan_grad(g, grad_ask(GRAD_TRAIN, f.vec4, grid, sorted, n, g.F, workspace, false), pull_knobs());
  if (!plan.want || plan.refuse) return MISO_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = zero_level_grads(g, plan.fill, st);
  if (e != hipSuccess) return (int)e;
  if (n == 0) {
    e = zero_loss_slots(loss_slots, st);
    if (e != hipSuccess) return (int)e;
  } else {
    const LossInK lin = loss_in(loss_type, weight_sdf, weight_fs, trunc_dist, loss_inputs, nullptr, loss_slots, n, n_live);
    e = launch_sdf_train(f.C, f.L, f.H, f.NH, gp, packed, x, n, sdf, perm, lin, plan.owned ? workspace : nullptr,
                         plan.owned, plan.scatter != 0, st);
    if (e != hipSuccess) return (int)e;
  }
  if (!plan.owned) return MISO_OK;
  return (int)launch_grad_pull(g, plan, pull_batch(sorted, workspace, nullptr, nullptr), st);
}

int miso_pair_latent(const miso_grid_t* dst_grid, const float* pose, const float* coords_src,
                     const float* feats_src, int64_t ld_feats, int64_t n, int loss_type, double* out,
                     void* stream) {
  if (n < 0 || !pose || !out || !mapping_loss_ok(loss_type)) return MISO_E_BADARG;
  if (!aligned(8, out)) return MISO_E_BADARG;      // fp64 atomics
  if (!set_if(n, coords_src, feats_src)) return MISO_E_BADARG;
  GridK g; bool v4;
  if (int rc = convert_grid(dst_grid, &g, true, &v4)) return rc;
  if (g.flags & (MISO_F_COORDS_NORMALIZED | MISO_F_ALIGN_CORNERS | MISO_F_PAD_BORDER)) return MISO_E_UNSUPPORTED;
  if (ld_feats < g.F) return MISO_E_BADARG;
  return (int)launch_pair_latent(g, v4, pose, coords_src, feats_src, ld_feats, n, loss_type, out,
                                 (hipStream_t)stream);
}

int miso_overlap_count(const float* pose, const float* coords_src, int64_t n, const float* bound_min,
                       const float* bound_max, float* count_out, void* stream) {
  if (n < 0 || !all_set(pose, bound_min, bound_max, count_out) || !set_if(n, coords_src)) return MISO_E_BADARG;
  if (!fits_fp32_count(n)) return MISO_E_TOOLARGE;
  return (int)launch_overlap_count(pose, coords_src, n, bound_min, bound_max, count_out, (hipStream_t)stream);
}

int miso_align_src_boxes(const float* coords, int64_t n, float* boxes, void* stream) {
  if (n < 0 || !set_if(n, coords, boxes)) return MISO_E_BADARG;
  return (int)launch_src_boxes(coords, n, boxes, (hipStream_t)stream);
}

int64_t miso_align_plan_bytes(int32_t n_pairs) {
  return n_pairs < 0 ? 0 : (int64_t)(n_pairs > 0 ? n_pairs : 1) * (int64_t)sizeof(AlignPairK);
}

// the loss types a residual has: latent L1 | L2; SDF against the source submap L1 | L2 | GM; against the measurement L2;
// the projected match L2
static bool align_loss_ok(int residual, int loss_type, float gm_scale) {
  if (residual == 0) return mapping_loss_ok(loss_type);
  if (residual == 1) return mapping_loss_ok(loss_type) || (loss_type == 3 && gm_scale > 0.0f);
  return (residual == 2 || residual == 3) && loss_type == 2;
}

// residual in 0..3, and the constraint that goes with it: 1 (point-to-plane) or 2 (point-to-point) with the projected
// match, 0 with every other residual
static bool align_residual_ok(int residual, int constraint) {
  if (residual < 0 || residual > 3) return false;
  return residual == 3 ? (constraint == 1 || constraint == 2) : constraint == 0;
}

int miso_align_plan_build(const miso_align_pair_t* pairs, miso_align_t* cfg, void* plan_host) {
  if (!cfg || cfg->n_pairs < 0 || cfg->n_submaps < 1 || cfg->n_submaps > 64) return MISO_E_BADARG;
  if (cfg->n_pairs > 0 && (!pairs || !plan_host)) return MISO_E_BADARG;
  const int residual = cfg->residual;
  if (!align_residual_ok(residual, cfg->constraint)) return MISO_E_BADARG;
  const bool reads_fsrc = !(residual == 3 && cfg->constraint == 2);      // (point-to-point has no column of its own)
  if (residual && (!cfg->mlp || !cfg->packed || !aligned(16, cfg->packed))) return MISO_E_BADARG;
  // (the latent form has always left the loss type to the iteration calls: kept)
  if ((residual || cfg->loss_type == 3) && !align_loss_ok(residual, cfg->loss_type, cfg->gm_scale)) return MISO_E_BADARG;
  int sdf_C = 0, sdf_L = 0, sdf_exact = -1;
  AlignPairK* out = reinterpret_cast<AlignPairK*>(plan_host);
  bool v4_all = true;
  int64_t max_n = 0, max_gate = 0, max_rows = 0;
  for (int p = 0; p < cfg->n_pairs; ++p) {
    const miso_align_pair_t& in = pairs[p];
    if (in.src < 0 || in.src >= cfg->n_submaps || in.dst < 0 || in.dst >= cfg->n_submaps || in.src == in.dst)
      return MISO_E_BADARG;
    if (in.n < 0 || in.gate_n < 0 || !set_if(in.n, in.coords_src)) return MISO_E_BADARG;
    if (reads_fsrc && !set_if(in.n, in.feats_src)) return MISO_E_BADARG;
    if (!fits_fp32_count(in.gate_n)) return MISO_E_TOOLARGE;
    if (residual == 2 && !fits_fp32_count(in.ld_feats)) return MISO_E_TOOLARGE;      // ld_feats: the source's full row count
    AlignPairK& d = out[p];
    memset(&d, 0, sizeof(d));
    bool v4;
    if (int rc = convert_grid(&in.dst_grid, &d.g, true, &v4)) return rc;
    if (d.g.flags & (MISO_F_COORDS_NORMALIZED | MISO_F_ALIGN_CORNERS | MISO_F_PAD_BORDER)) return MISO_E_UNSUPPORTED;
    if (residual) {
      // one kernel instantiation and one arithmetic serve every pair of the launch
      int C_, L_, H_, NH_;
      if (int rc = fused_shape(d.g, v4, cfg->mlp, &C_, &L_, &H_, &NH_)) return rc;
      if (!pair_sdf_covered(C_, L_, H_, NH_)) return MISO_E_UNSUPPORTED;
      const int exact = (d.g.flags & MISO_F_EXACT_F32) ? 1 : 0;
      if (sdf_exact >= 0 && (C_ != sdf_C || L_ != sdf_L || exact != sdf_exact)) return MISO_E_UNSUPPORTED;
      sdf_C = C_; sdf_L = L_; sdf_exact = exact;
      // the pitch of the column read: ref (1), the source normals (3); residual 2: the full row count instead
      if (reads_fsrc && in.ld_feats < (residual == 2 ? in.n : (residual == 3 ? 3 : 1))) return MISO_E_BADARG;
    } else if (in.ld_feats < d.g.F) {
      return MISO_E_BADARG;
    }
    v4_all = v4_all && v4;
    d.p = in.coords_src; d.fsrc = in.feats_src; d.ld = residual == 2 ? 1 : in.ld_feats; d.n = in.n;
    d.gate_p = in.gate_n > 0 ? in.gate_coords : nullptr; d.gate_n = in.gate_n;
    if (in.gate_n > 0 && in.gate_axis[0]) {
      if (!in.gate_axis[1] || !in.gate_axis[2]) return MISO_E_BADARG;
      int64_t prod = 1;
      for (int a = 0; a < 3; ++a) {
        if (in.gate_dims[a] < 1) return MISO_E_BADARG;
        d.gate_ax[a] = in.gate_axis[a]; d.gate_dim[a] = in.gate_dims[a];
        prod *= in.gate_dims[a];
      }
      if (prod != in.gate_n) return MISO_E_BADARG;
      d.gate_p = in.gate_axis[0];      // non-null marks the gate as on; the lattice path does not read it as points
      if ((int64_t)in.gate_dims[1] * in.gate_dims[2] > max_rows) max_rows = (int64_t)in.gate_dims[1] * in.gate_dims[2];
    } else if (in.gate_n > 0 && !in.gate_coords) {
      return MISO_E_BADARG;
    }
    d.src = in.src; d.dst = in.dst;
    d.n_ch = residual == 0 ? (float)d.g.F : (residual == 1 ? 1.0f : (residual == 2 ? (float)in.ld_feats
                                                                                    : (cfg->constraint == 2 ? 3.0f : 1.0f)));
    d.boxes = in.n > 0 ? in.src_boxes : nullptr;
    if (in.n > max_n) max_n = in.n;
    if (d.gate_p && !d.gate_ax[0] && in.gate_n > max_gate) max_gate = in.gate_n;      // point-list gates only (grid sizing)
  }
  cfg->vec4 = v4_all ? 1 : 0;
  cfg->max_n = max_n;
  cfg->max_gate_n = max_gate;
  cfg->max_gate_rows = max_rows;
  cfg->sdf_shape = sdf_exact >= 0 ? (sdf_C | (sdf_L << 8) | (sdf_exact << 16)) : 0;
  return MISO_OK;
}

int64_t miso_align_state_layout(int32_t n_submaps, int32_t n_pairs, int32_t ring_iters, int32_t save_poses,
                                int64_t* offsets) {
  if (n_submaps < 1 || n_submaps > 64 || n_pairs < 0 || ring_iters < 0) return 0;
  const AlignLayout L = align_layout(n_submaps, n_pairs, ring_iters, save_poses);
  if (offsets) {
    const int64_t o[12] = {L.params, L.pose, L.out, L.cnt, L.pair_loss, L.flat, L.adam_m, L.adam_v, L.ctrl, L.ring,
                           L.ring_row, L.adam_t};
    for (int i = 0; i < 12; ++i) offsets[i] = o[i];
  }
  return L.total;
}

static int align_k(const miso_align_t* c, AlignK* k) {
  if (!c || c->n_submaps < 1 || c->n_submaps > 64 || c->n_pairs < 0 || c->ring_iters < 0) return MISO_E_BADARG;
  if (!c->R0 || !c->t0 || !c->state || (c->n_pairs > 0 && !c->plan)) return MISO_E_BADARG;
  if (!align_residual_ok(c->residual, c->constraint) || !align_loss_ok(c->residual, c->loss_type, c->gm_scale)) return MISO_E_BADARG;
  if (!aligned(16, c->state)) return MISO_E_BADARG;
  if (c->residual && (!c->mlp || !c->packed || !aligned(16, c->packed))) return MISO_E_BADARG;
  memset(k, 0, sizeof(*k));
  k->residual = c->residual;
  if (c->residual && c->n_pairs > 0) {      // (a plan without a pair launches no pair stage)
    PairSdfK& f = k->sdf;
    f.C = c->sdf_shape & 255; f.L = (c->sdf_shape >> 8) & 255; f.exact = ((c->sdf_shape >> 16) & 1) != 0;
    f.H = c->mlp->hidden_dim; f.NH = c->mlp->n_linear - 2;
    f.packed = c->packed; f.gm_scale = c->gm_scale; f.constraint = c->constraint;
    if (c->mlp->in_dim != f.C * f.L || !pair_sdf_covered(f.C, f.L, f.H, f.NH)) return MISO_E_UNSUPPORTED;
  }
  k->S = c->n_submaps; k->P = c->n_pairs; k->loss_type = c->loss_type; k->ring_iters = c->ring_iters;
  k->save_poses = c->save_poses;
  k->align_weight = c->align_weight; k->overlap_thresh = c->overlap_thresh; k->reg_weight = c->reg_weight;
  k->reg_rad = c->reg_thresh_rad; k->reg_m = c->reg_thresh_m; k->rel_thresh = c->rel_change_thresh;
  k->lr = c->lr; k->b1 = c->beta1; k->b2 = c->beta2; k->eps = c->eps;
  k->R0 = c->R0; k->t0 = c->t0; k->plan = reinterpret_cast<const AlignPairK*>(c->plan); k->state = c->state;
  k->L = align_layout(k->S, k->P, k->ring_iters, k->save_poses);
  return MISO_OK;
}

int miso_align_iteration_a(const miso_align_t* cfg, void* stream) {
  AlignK k;
  if (int rc = align_k(cfg, &k)) return rc;
  return (int)launch_align_a(k, cfg->max_n, cfg->max_gate_n, cfg->max_gate_rows, cfg->vec4 != 0, cfg->poses_ready != 0,
                             (hipStream_t)stream);
}

int miso_align_iteration_b(const miso_align_t* cfg, void* stream) {
  AlignK k;
  if (int rc = align_k(cfg, &k)) return rc;
  return (int)launch_align_b(k, (hipStream_t)stream);
}

int miso_lm_normal_eq(const float* coords_frame, const float* R_frame, const float* grad_sdf_x,
                      const float* sdf, const float* target, int64_t n, int loss_type, float gm_scale,
                      float* out, void* stream) {
  if (n < 0 || !out || !R_frame || !set_if(n, coords_frame, grad_sdf_x, sdf, target)) return MISO_E_BADARG;
  if (loss_type != 2 && loss_type != 3) return MISO_E_UNSUPPORTED;
  if (loss_type == 3 && !(gm_scale > 0.0f)) return MISO_E_BADARG;
  return (int)launch_lm_normal_eq(coords_frame, R_frame, grad_sdf_x, sdf, target, n, loss_type, gm_scale, out,
                                  (hipStream_t)stream);
}

static int lm_track_args(const miso_grid_t* grid, const miso_lm_track_t* a, LmTrackK* out) {
  LmTrackK& k = *out;
  memset(&k, 0, sizeof(k));
  k.x = a->coords_frame; k.gt = a->target; k.valid = a->valid; k.frame_ids = a->frame_ids;
  k.s_gt = a->stride_target; k.s_valid = a->stride_valid; k.s_fid = a->stride_frame_ids;
  k.valid_is_bool = a->valid_is_bool; k.n = a->n; k.kf = a->keyframe_id; k.trunc = a->trunc_dist;
  k.Rwk = a->R_base; k.twk = a->t_base; k.dr = a->rot_correction; k.dt = a->trans_correction;
  k.pose = a->pose; k.xw = a->coords_world; k.sums = a->sums; k.info = a->info; k.clean = a->sanitized;
  for (int i = 0; i < 3; ++i) { k.bmin[i] = grid->bound_min[i]; k.bmax[i] = grid->bound_max[i]; }
  k.lm_lambda = a->lm_lambda;
  return MISO_OK;
}

// after the head (pose + transform) has run: the later kernels read the sanitised copies
static void lm_track_use_clean(LmTrackK* k) {
  if (!k->clean) return;
  k->x = k->clean; k->gt = k->clean + 3 * k->n; k->s_gt = 1;
  k->valid = k->clean + 4 * k->n; k->s_valid = 1; k->valid_is_bool = 0;
  k->clean = nullptr;
}

int miso_track_adam_step(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const miso_track_adam_t* t,
                         void* stream) {
  if (!t || !grid) return MISO_E_BADARG;
  const miso_lm_track_t* a = &t->s;
  if (!lm_track_ok(a, t->grad_pred)) return MISO_E_BADARG;
  if (!t->adam_table || t->adam_table_len < 1 || !t->state || t->ring_len < 0 || !set_if(t->ring_len, t->loss_ring))
    return MISO_E_BADARG;
  if (t->loss_type < 1 || t->loss_type > 3) return MISO_E_UNSUPPORTED;
  if (t->loss_type == 3 && !(t->gm_scale > 0.0f)) return MISO_E_BADARG;
  if (has_grad_buffers(grid)) return MISO_E_BADARG;
  TrackAdamK k;
  memset(&k, 0, sizeof(k));
  lm_track_args(grid, a, &k.s);
  k.loss_type = t->loss_type; k.weight_sdf = t->weight_sdf; k.gm_scale = t->gm_scale;
  k.gpred = t->grad_pred; k.gx = a->grad; k.sdf = a->sdf;
  k.table = reinterpret_cast<const AdamScalars*>(t->adam_table); k.table_len = t->adam_table_len;
  k.state = t->state; k.ring = t->loss_ring; k.ring_len = t->ring_len;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = (int)launch_lm_track_head(k.s, st)) return rc;
  lm_track_use_clean(&k.s);
  if (a->n > 0) {
    if (int rc = miso_sdf_fwd(grid, mlp, packed, a->coords_world, nullptr, a->n, a->sdf, a->relu_mask, stream)) return rc;
    if (int rc = (int)launch_track_loss(k, st)) return rc;
    if (int rc = miso_sdf_bwd(grid, mlp, packed, a->coords_world, nullptr, a->n, t->grad_pred, a->relu_mask, a->grad, nullptr, stream))
      return rc;
  }
  return (int)launch_track_tail(k, st);
}

int miso_lm_track_step(const miso_grid_t* grid, const miso_mlp_t* mlp, const float* packed, const miso_lm_track_t* a,
                       void* stream) {
  if (!a || !lm_track_ok(a, a->ones)) return MISO_E_BADARG;
  if (a->loss_type != 2 && a->loss_type != 3) return MISO_E_UNSUPPORTED;
  if (a->loss_type == 3 && !(a->gm_scale > 0.0f)) return MISO_E_BADARG;
  if (!grid || has_grad_buffers(grid)) return MISO_E_BADARG;
  LmTrackK k;
  lm_track_args(grid, a, &k);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = (int)launch_lm_track_head(k, st)) return rc;
  lm_track_use_clean(&k);
  if (a->n > 0) {
    if (int rc = miso_sdf_fwd(grid, mlp, packed, a->coords_world, nullptr, a->n, a->sdf, a->relu_mask, stream)) return rc;
    if (int rc = miso_sdf_bwd(grid, mlp, packed, a->coords_world, nullptr, a->n, a->ones, a->relu_mask, a->grad, nullptr, stream)) return rc;
  }
  return (int)launch_lm_track_tail(k, a->grad, a->sdf, a->loss_type, a->gm_scale, st);
}

int64_t miso_pull_queue_ints(int64_t n) { return n < 0 ? 0 : pull_queue_ints(n); }

int64_t miso_sample_rays_workspace_bytes(int64_t n_rays, int32_t n_frames) {
  if (n_rays < 0 || n_frames < 0) return 0;
  return (int64_t)sample_rays_workspace_bytes(n_rays, n_frames);
}

int miso_sample_rays(const miso_ray_frames_t* f, const miso_ray_sampling_t* c, int64_t n_rays, const int64_t* pix_b,
                     const int64_t* pix_h, const int64_t* pix_w, const float* u, const float* g, void* workspace,
                     float* coords_frame, int64_t* sample_frame_ids, float* aux, float* pc_world, float* z_vals,
                     int32_t* counts, void* stream) {
  if (!f || !c || n_rays < 0 || !counts) return MISO_E_BADARG;
  if (c->n_strat < 0 || c->n_surf < 0 || c->n_strat + c->n_surf < 1) return MISO_E_BADARG;
  if (c->n_strat > MISO_RAY_MAX_BINS) return MISO_E_UNSUPPORTED;
  const int64_t S = c->n_strat + c->n_surf;
  if (!fits32(n_rays * S)) return MISO_E_TOOLARGE;
  if (n_rays > 0) {
    if (!f->depth || !f->T_WC || !f->R_wk || !f->t_wk || f->n_frames < 1 || f->H < 1 || f->W < 1) return MISO_E_BADARG;
    if (!pix_h || !pix_w || !workspace || !coords_frame || !sample_frame_ids || !aux) return MISO_E_BADARG;
    if (!pix_b && c->rays_per_frame < 1) return MISO_E_BADARG;
    if ((c->n_strat > 0 && !u) || (c->n_surf > 1 && !g)) return MISO_E_BADARG;
    if (!aligned(16, aux)) return MISO_E_BADARG;
  }
  float lin[MISO_RAY_MAX_BINS + 1];
  if (c->bin_edges) {
    for (int i = 0; i <= c->n_strat; ++i) lin[i] = c->bin_edges[i];
  } else {   // at::linspace's two-sided float formula
    const int steps = c->n_strat + 1;
    const float step = steps > 1 ? 1.0f / (float)(steps - 1) : 0.0f;
    for (int i = 0; i < steps; ++i) lin[i] = i < steps / 2 ? step * (float)i : 1.0f - step * (float)(steps - 1 - i);
  }
  return (int)launch_sample_rays(*f, *c, lin, n_rays, pix_b, pix_h, pix_w, u, g, workspace, coords_frame,
                                 sample_frame_ids, aux, pc_world, z_vals, counts, (hipStream_t)stream);
}

int miso_mapping_loss(int loss_type, float weight_sdf, float weight_fs, float trunc_dist,
                      const float* pred, const float* target, const float* valid, const float* sign,
                      const float* weight, int64_t n, float* grad_pred, float* grad_pred_fs,
                      float* loss_out, void* stream) {
  if (n < 0 || !mapping_loss_ok(loss_type) || !loss_out || !set_if(n, pred, target, grad_pred)) return MISO_E_BADARG;
  return (int)launch_mapping_loss(loss_type, weight_sdf, weight_fs, trunc_dist, pred, target, valid,
                                  sign, weight, n, grad_pred, grad_pred_fs, loss_out, (hipStream_t)stream);
}

int miso_adam_dense(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                    double lr, double beta1, double beta2, double eps, int32_t step, int zero_grad,
                    void* stream) {
  if (numel < 0 || step < 1 || !set_if(numel, param, grad, exp_avg, exp_avg_sq)) return MISO_E_BADARG;
  return (int)launch_adam(param, grad, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, step,
                          zero_grad, (hipStream_t)stream);
}

// `when` is the host form (table NULL, a step >= 1) or the device form (table, its length, the count on the device)
int miso_adam_step(const miso_adam_tensor_t* tensors, int32_t n_tensors, const miso_adam_when_t* when, const float* guard,
                   void* stream) {
  if (!adam_tensors_ok(tensors, n_tensors) || !when) return MISO_E_BADARG;
  if (when->table ? when->table_len < 1 || !when->step_dev : when->step < 1) return MISO_E_BADARG;
  return (int)launch_adam_step(tensors, n_tensors, *when, guard, (hipStream_t)stream);
}

int miso_adam_scalars_table(double lr, double beta1, double beta2, double eps, int32_t first_step, int32_t count,
                            float* host_out) {
  if (first_step < 1 || count < 0 || (count > 0 && !host_out)) return MISO_E_BADARG;
  adam_scalars_table(lr, beta1, beta2, eps, first_step, count, host_out);
  return MISO_OK;
}

int miso_loss_total_bump(const float* loss_slots, int32_t n_floats, float* total, int32_t* step, float* host_ring,
                         int32_t ring_len, void* stream) {
  if (!loss_slots || n_floats < 1 || !total) return MISO_E_BADARG;
  if (host_ring && (!step || ring_len < 1 || (ring_len & (ring_len - 1)))) return MISO_E_BADARG;
  return (int)launch_loss_total_bump(loss_slots, n_floats, total, step, host_ring, host_ring ? ring_len : 0,
                                     (hipStream_t)stream);
}

int miso_adam_bump(int32_t* step, const float* guard, void* stream) {
  if (!step) return MISO_E_BADARG;
  return (int)launch_adam_bump(step, guard, (hipStream_t)stream);
}

int miso_mapping_batch(const float* R, const float* t, int32_t n_poses, const int64_t* table, int64_t table_len,
                       const int64_t* frame_ids, const float* coords_frame, const float* target, const void* valid,
                       const float* sign, const float* weight, const int64_t* col_strides, int valid_is_bool, int64_t n,
                       float* coords_world, float* loss_rows, int sanitize, void* stream) {
  if (n < 0 || n_poses < 1 || table_len < 1 || !R || !t || !table) return MISO_E_BADARG;
  if (col_strides)
    for (int i = 0; i < 4; ++i)
      if (col_strides[i] < 0) return MISO_E_BADARG;
  if (!set_if(n, frame_ids, coords_frame, target, coords_world, loss_rows) || !aligned(16, loss_rows)) return MISO_E_BADARG;
  return (int)launch_mapping_batch(R, t, n_poses, table, table_len, frame_ids, coords_frame, target, valid, sign, weight,
                                   n, coords_world, loss_rows, col_strides, valid_is_bool, sanitize, (hipStream_t)stream);
}

int miso_mapping_loss_rows(int loss_type, float weight_sdf, float weight_fs, float trunc_dist, const float* pred,
                           const float* loss_rows, int64_t n, float* grad_pred, float* loss_out, void* stream) {
  if (!mapping_loss_ok(loss_type) || n < 0 || !loss_out || !set_if(n, pred, loss_rows, grad_pred) || !aligned(16, loss_rows))
    return MISO_E_BADARG;
  return (int)launch_mapping_loss_rows(loss_type, weight_sdf, weight_fs, trunc_dist, pred, loss_rows, n, grad_pred,
                                       loss_out, (hipStream_t)stream);
}

int miso_rigid_by_index(const float* R, const float* t, const int64_t* idx, const float* x, int64_t n, int32_t n_poses,
                        int transpose, float* y, void* stream) {
  if (n < 0 || n_poses < 1 || !R || !set_if(n, idx, x, y)) return MISO_E_BADARG;
  return (int)launch_rigid_by_index(R, t, idx, x, n, n_poses, transpose, y, (hipStream_t)stream);
}

int64_t miso_mc_words(int32_t nx, int32_t ny, int32_t nz) {
  if (mc_check_dims(nx, ny, nz)) return -1;
  return mc_words(nx, ny, nz);
}

int miso_grid_pool_avg(const float* coords, const float* features, int64_t n, int32_t d, int64_t ld_features,
                       const float* bound_min, float cell_size, int32_t nx, int32_t ny, int32_t nz, float* pooled,
                       int32_t* counts, void* stream) {
  if (n < 0 || d < 1 || nx < 1 || ny < 1 || nz < 1 || !bound_min || !pooled || !counts || !(cell_size > 0.0f)) return MISO_E_BADARG;
  if (n > 0 && (!coords || !features || ld_features < d)) return MISO_E_BADARG;
  if (!fits32((int64_t)nx * ny * nz * d)) return MISO_E_TOOLARGE;
  return (int)launch_grid_pool_avg(coords, features, n, d, ld_features, bound_min, cell_size, nx, ny, nz, pooled, counts,
                                   (hipStream_t)stream);
}

// ---- voxel down-sampling (voxel.hip) -------------------------------------------------------------------------------------
int64_t miso_voxel_down_workspace_bytes(int64_t capacity) {
  if (capacity < 0 || !fits_voxel_key(capacity)) return 0;
  return voxel_down_workspace_bytes(capacity);
}

int miso_voxel_down_sample(const float* points, int64_t ld, int64_t capacity, const int32_t* n_live, float voxel_size,
                           void* workspace, int64_t* out_idx, int32_t* out_count, void* stream) {
  if (capacity < 0 || ld < 3 || !out_count || !(voxel_size > 0.0f) || !(voxel_size < __builtin_huge_valf()))
    return MISO_E_BADARG;
  if (!fits_voxel_key(capacity)) return MISO_E_TOOLARGE;
  if (capacity == 0) return (int)launch_zero_words(out_count, 1, (hipStream_t)stream);
  if (!all_set(points, workspace, out_idx) || !aligned(8, workspace)) return MISO_E_BADARG;
  return (int)launch_voxel_down_sample(points, ld, capacity, n_live, voxel_size, workspace, out_idx, out_count,
                                       (hipStream_t)stream);
}

int miso_voxel_select_rows(const float* src_coords, const int64_t* src_ids, const float* src_aux, const int64_t* out_idx,
                           const int32_t* out_count, int64_t capacity, float* dst_coords, int64_t* dst_ids, float* dst_aux,
                           int32_t* live_rows, void* stream) {
  if (capacity < 0 || !out_count || !live_rows) return MISO_E_BADARG;
  if (!fits_voxel_key(capacity)) return MISO_E_TOOLARGE;
  if (!set_if(capacity, src_coords, src_ids, src_aux, out_idx, dst_coords, dst_ids, dst_aux)) return MISO_E_BADARG;
  if (!aligned(16, src_aux, dst_aux)) return MISO_E_BADARG;
  if (capacity > 0 && (src_coords == dst_coords || src_ids == dst_ids || src_aux == dst_aux)) return MISO_E_BADARG;
  return (int)launch_voxel_select_rows(src_coords, src_ids, src_aux, out_idx, out_count, capacity, dst_coords, dst_ids,
                                       dst_aux, live_rows, (hipStream_t)stream);
}

// ---- exact nearest neighbour (nn.hip) --------------------------------------------------------------------------------------
int miso_nn_plan(const float* bound_min, const float* bound_max, float cell, int64_t n_tgt, int32_t max_rings,
                 miso_nn_plan_t* plan) {
  const float inf = __builtin_huge_valf();
  if (!plan || !bound_min || !bound_max || n_tgt < 0 || max_rings < 0 || max_rings > MISO_NN_MAX_RINGS) return MISO_E_BADARG;
  if (!(cell > 0.0f) || !(cell < inf)) return MISO_E_BADARG;
  if (!fits32(n_tgt)) return MISO_E_TOOLARGE;
  memset(plan, 0, sizeof(*plan));
  plan->n_tgt = n_tgt; plan->max_rings = max_rings; plan->cell = cell;
  plan->dims[0] = plan->dims[1] = plan->dims[2] = 1; plan->cells = 1;
  if (n_tgt == 0) return MISO_OK;
  // dims in the kernels' arithmetic (fp32 difference, fp32 division, floor): the cell index of the largest coordinate is
  // dims - 1 without the clamp
  float ext[3];
  double mag = 0.0;
  for (int a = 0; a < 3; ++a) {
    if (!(fabsf(bound_min[a]) < inf) || !(fabsf(bound_max[a]) < inf) || bound_max[a] < bound_min[a]) return MISO_E_BADARG;
    ext[a] = bound_max[a] - bound_min[a];
    if (!(ext[a] < inf)) return MISO_E_BADARG;
    plan->bound_min[a] = bound_min[a];
  }
  float c = cell;
  for (;;) {
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) cells *= (double)floorf(ext[a] / c) + 1.0;
    if (cells <= (double)MISO_NN_MAX_CELLS) break;
    c *= 2.0f;
    if (!(c < inf)) return MISO_E_BADARG;
  }
  plan->cell = c;
  plan->cells = 1;
  for (int a = 0; a < 3; ++a) {
    plan->dims[a] = (int32_t)floorf(ext[a] / c) + 1;
    plan->cells *= plan->dims[a];
    const double top = fmax(fabs((double)bound_min[a]), fabs((double)bound_min[a] + (double)plan->dims[a] * c));
    mag = fmax(mag, top + (double)plan->dims[a] * c);
  }
  plan->coord_mag = (float)fmin(mag * (1.0 + 1e-6), 3.0e38);
  return MISO_OK;
}

int64_t miso_nn_workspace_bytes(const miso_nn_plan_t* plan) {
  return nn_plan_ok(plan) ? nn_workspace_bytes(*plan) : 0;
}

int miso_nn_build(const miso_nn_plan_t* plan, const float* tgt, int64_t ld, void* workspace, void* stream) {
  if (!nn_plan_ok(plan) || ld < 3) return MISO_E_BADARG;
  if (plan->n_tgt == 0) return MISO_OK;
  if (!tgt || !index_ready(plan->n_tgt, workspace)) return MISO_E_BADARG;
  return (int)launch_nn_build(*plan, tgt, ld, workspace, (hipStream_t)stream);
}

int miso_nn_query(const miso_nn_plan_t* plan, void* workspace, const float* src, int64_t ld, int64_t n, float* out_d2,
                  int64_t* out_idx, int32_t* stats, void* stream) {
  if (!nn_plan_ok(plan) || !stats) return MISO_E_BADARG;
  if (int rc = check_cloud(src, ld, n, out_d2, out_idx)) return rc;
  if (!index_ready(plan->n_tgt, workspace)) return MISO_E_BADARG;
  return (int)launch_nn_query(*plan, workspace, src, ld, n, out_d2, out_idx, stats, (hipStream_t)stream);
}

// targets and queries both in the caller's arrays
static int check_cloud_pair(const float* tgt, int64_t ld_t, int64_t m, const float* src, int64_t ld_s, int64_t n, float* out_d2,
                            int64_t* out_idx) {
  if (int rc = check_cloud(tgt, ld_t, m)) return rc;
  return check_cloud(src, ld_s, n, out_d2, out_idx);
}

int miso_nn_all_pairs(const float* tgt, int64_t ld_t, int64_t m, const float* src, int64_t ld_s, int64_t n, float* out_d2,
                      int64_t* out_idx, void* stream) {
  if (int rc = check_cloud_pair(tgt, ld_t, m, src, ld_s, n, out_d2, out_idx)) return rc;
  return (int)launch_nn_all_pairs(tgt, ld_t, m, src, ld_s, n, out_d2, out_idx, (hipStream_t)stream);
}

// ---- exact k nearest neighbours on the index (knn.hip) -------------------------------------------------------------------
int miso_nn_knn(const miso_nn_plan_t* plan, void* workspace, const float* src, int64_t ld, int64_t n, int32_t k, float* out_d2,
                int64_t* out_idx, int32_t* stats, void* stream) {
  if (!nn_plan_ok(plan) || !nn_k_ok(k) || !stats) return MISO_E_BADARG;
  if (int rc = check_cloud(src, ld, n, out_d2, out_idx)) return knn_code(rc);
  if (!index_ready(plan->n_tgt, workspace)) return MISO_E_BADARG;
  return (int)launch_nn_knn(*plan, workspace, src, ld, n, k, out_d2, out_idx, stats, (hipStream_t)stream);
}

int miso_nn_knn_all_pairs(const float* tgt, int64_t ld_t, int64_t m, const float* src, int64_t ld_s, int64_t n, int32_t k,
                          float* out_d2, int64_t* out_idx, void* stream) {
  if (!nn_k_ok(k)) return MISO_E_BADARG;
  if (int rc = check_cloud_pair(tgt, ld_t, m, src, ld_s, n, out_d2, out_idx)) return knn_code(rc);
  return (int)launch_nn_knn_all_pairs(tgt, ld_t, m, src, ld_s, n, k, out_d2, out_idx, (hipStream_t)stream);
}

int miso_nn_knn_normals(const miso_nn_plan_t* plan, void* workspace, const float* pts, int64_t ld, int64_t n, int32_t k,
                        float* normals, int32_t* counts, void* stream) {
  if (!nn_plan_ok(plan) || !nn_k_ok(k)) return MISO_E_BADARG;
  if (int rc = check_cloud(pts, ld, n, normals, counts)) return knn_code(rc);
  if (!index_ready(plan->n_tgt, workspace)) return MISO_E_BADARG;
  return (int)launch_nn_knn_normals(*plan, workspace, pts, ld, n, k, normals, counts, (hipStream_t)stream);
}

// ---- ICP and normals on the index (icp.hip) ----------------------------------------------------------------------------------
int miso_icp_transform(const float* src, int64_t ld, int64_t n, const float* pose, float* out, void* stream) {
  if (!pose) return MISO_E_BADARG;
  if (int rc = check_cloud(src, ld, n, out)) return rc;
  return (int)launch_icp_transform(pose, src, ld, n, out, (hipStream_t)stream);
}

int64_t miso_icp_workspace_bytes(int64_t n) { return n < 0 ? 0 : icp_workspace_bytes(n); }

int miso_icp_sums(const float* moved, const float* d2, const int64_t* idx, int64_t n, const float* tgt, int64_t ld_t,
                  int64_t m, const float* normals, int64_t ld_n, double max_dist, int32_t kind, int32_t loss,
                  double tukey_k, const double* origin, void* workspace, double* out, void* stream) {
  if (n < 0 || m < 0 || ld_t < 3 || !workspace || !out || !aligned(8, workspace, out)) return MISO_E_BADARG;
  if (!fits32(n) || !fits32(m)) return MISO_E_TOOLARGE;
  if (kind != MISO_ICP_POINT_TO_POINT && kind != MISO_ICP_POINT_TO_PLANE) return MISO_E_BADARG;
  if (loss != MISO_ICP_LOSS_L2 && loss != MISO_ICP_LOSS_TUKEY) return MISO_E_BADARG;
  if (!(max_dist >= 0.0) || (loss == MISO_ICP_LOSS_TUKEY && !(tukey_k > 0.0))) return MISO_E_BADARG;
  if (n > 0 && (!moved || !d2 || !idx || (m > 0 && !tgt))) return MISO_E_BADARG;
  if (kind == MISO_ICP_POINT_TO_PLANE && n > 0 && m > 0 && (!normals || ld_n < 3)) return MISO_E_BADARG;
  return (int)launch_icp_sums(moved, d2, idx, n, tgt, ld_t, m, normals, ld_n, max_dist, kind, loss, tukey_k, origin, workspace,
                              out, (hipStream_t)stream);
}

int miso_nn_normals(const miso_nn_plan_t* plan, const void* workspace, const float* pts, int64_t ld, int64_t n,
                    double radius, float* normals, int32_t* counts, void* stream) {
  if (!nn_plan_ok(plan) || !(radius > 0.0) || !(radius < 1e30)) return MISO_E_BADARG;
  if (int rc = check_cloud(pts, ld, n, normals, counts)) return rc;
  if (!index_ready(plan->n_tgt, workspace)) return MISO_E_BADARG;
  return (int)launch_nn_normals(*plan, workspace, pts, ld, n, radius, normals, counts, (hipStream_t)stream);
}

// ---- ray casting against a triangle mesh (mesh.hip) ---------------------------------------------------------------------------
int miso_mesh_plan(const float* bound_min, const float* bound_max, float cell, int64_t n_tri, miso_mesh_plan_t* plan) {
  if (!plan || n_tri < 0) return MISO_E_BADARG;
  if (!fits32(n_tri)) return MISO_E_TOOLARGE;
  // the grid is the nearest-neighbour index's: the same dims, doubling and coord_mag (MISO_MESH_MAX_CELLS == MISO_NN_MAX_CELLS)
  static_assert(MISO_MESH_MAX_CELLS == MISO_NN_MAX_CELLS, "one grid plan");
  miso_nn_plan_t g;
  const int rc = miso_nn_plan(bound_min, bound_max, cell, n_tri, 0, &g);
  if (rc != MISO_OK) return rc;
  memset(plan, 0, sizeof(*plan));
  for (int a = 0; a < 3; ++a) { plan->bound_min[a] = g.bound_min[a]; plan->dims[a] = g.dims[a]; }
  plan->cell = g.cell; plan->coord_mag = g.coord_mag; plan->widen = 0x1p-17f * g.coord_mag;
  plan->n_tri = n_tri; plan->cells = g.cells;
  return MISO_OK;
}

int64_t miso_mesh_workspace_bytes(const miso_mesh_plan_t* plan) {
  return mesh_plan_ok(plan) ? mesh_workspace_bytes(*plan) : 0;
}

int miso_mesh_count(const miso_mesh_plan_t* plan, const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris,
                    int64_t ld_t, void* workspace, int64_t* entries, void* stream) {
  if (!mesh_plan_ok(plan) || !entries || !aligned(8, entries)) return MISO_E_BADARG;
  if (int rc = check_mesh_arrays(verts, ld_v, n_vert, tris, ld_t, plan->n_tri)) return rc;
  if (!index_ready(plan->n_tri, workspace)) return MISO_E_BADARG;
  return (int)launch_mesh_count(*plan, verts, ld_v, n_vert, tris, ld_t, workspace, entries, (hipStream_t)stream);
}

int miso_mesh_build(const miso_mesh_plan_t* plan, void* workspace, int32_t* lists, int64_t capacity, void* stream) {
  if (!mesh_index_ok(plan, workspace, lists, capacity)) return MISO_E_BADARG;
  if (capacity > MISO_MESH_MAX_ENTRIES) return MISO_E_TOOLARGE;
  if (plan->n_tri == 0) return MISO_OK;
  return (int)launch_mesh_build(*plan, workspace, lists, capacity, (hipStream_t)stream);
}

int miso_mesh_cast_rays(const miso_mesh_plan_t* plan, const void* workspace, const int32_t* lists, int64_t capacity,
                        const float* origins, int64_t ld_o, const float* dirs, int64_t ld_d, int64_t n, float t_min,
                        float t_max, float* out_t, int64_t* out_tri, int64_t* stats, void* stream) {
  if (!mesh_index_ok(plan, workspace, lists, capacity) || !aligned(8, stats)) return MISO_E_BADARG;
  if (capacity > MISO_MESH_MAX_ENTRIES) return MISO_E_TOOLARGE;
  if (int rc = check_rays(origins, ld_o, dirs, ld_d, n, out_t, out_tri)) return rc;
  return (int)launch_mesh_cast_rays(*plan, workspace, lists, capacity, origins, ld_o, dirs, ld_d, n, t_min, t_max, out_t, out_tri,
                                    stats, (hipStream_t)stream);
}

int miso_mesh_cast_rays_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t,
                            int64_t n_tri, const float* origins, int64_t ld_o, const float* dirs, int64_t ld_d, int64_t n,
                            float t_min, float t_max, float* out_t, int64_t* out_tri, void* stream) {
  if (int rc = check_mesh_arrays(verts, ld_v, n_vert, tris, ld_t, n_tri)) return rc;
  if (int rc = check_rays(origins, ld_o, dirs, ld_d, n, out_t, out_tri)) return rc;
  return (int)launch_mesh_cast_rays_all(verts, ld_v, n_vert, tris, ld_t, n_tri, origins, ld_o, dirs, ld_d, n, t_min, t_max, out_t,
                                        out_tri, (hipStream_t)stream);
}

// ---- closest triangle and crossing counts on the mesh index (mesh_sdf.hip) ----------------------------------------------------
int miso_mesh_closest(const miso_mesh_plan_t* plan, const void* workspace, const int32_t* lists, int64_t capacity,
                      const miso_mesh_plan_t* plan_far, const void* workspace_far, const int32_t* lists_far, int64_t capacity_far,
                      const float* pts, int64_t ld_p, int64_t n, float* out_d2, int64_t* out_tri, float* out_vw, int64_t* stats,
                      void* stream) {
  if (!mesh_index_ok(plan, workspace, lists, capacity) || !aligned(8, stats, out_vw)) return MISO_E_BADARG;
  // the far set is one more index of the SAME triangles (the kernel reads the rows of the first), or absent as a whole
  if (plan_far ? (!mesh_index_ok(plan_far, workspace_far, lists_far, capacity_far) || plan_far->n_tri != plan->n_tri || plan_far->reserved < 0)
               : (workspace_far || lists_far || capacity_far != 0))
    return MISO_E_BADARG;
  if (capacity > MISO_MESH_MAX_ENTRIES || capacity_far > MISO_MESH_MAX_ENTRIES) return MISO_E_TOOLARGE;
  if (int rc = check_cloud(pts, ld_p, n, out_d2, out_tri)) return rc;
  return (int)launch_mesh_closest(*plan, workspace, lists, capacity, plan_far, workspace_far, lists_far, capacity_far, pts, ld_p, n,
                                  out_d2, out_tri, out_vw, stats, (hipStream_t)stream);
}

int miso_mesh_closest_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t, int64_t n_tri,
                          const float* pts, int64_t ld_p, int64_t n, float* out_d2, int64_t* out_tri, float* out_vw, void* stream) {
  if (!aligned(8, out_vw)) return MISO_E_BADARG;
  if (int rc = check_mesh_arrays(verts, ld_v, n_vert, tris, ld_t, n_tri)) return rc;
  if (int rc = check_cloud(pts, ld_p, n, out_d2, out_tri)) return rc;
  return (int)launch_mesh_closest_all(verts, ld_v, n_vert, tris, ld_t, n_tri, pts, ld_p, n, out_d2, out_tri, out_vw, (hipStream_t)stream);
}

int miso_mesh_count_hits(const miso_mesh_plan_t* plan, const void* workspace, const int32_t* lists, int64_t capacity,
                         const float* origins, int64_t ld_o, const float* dirs, int64_t ld_d, int64_t n, float t_min, float t_max,
                         int32_t* out_count, void* stream) {
  if (!mesh_index_ok(plan, workspace, lists, capacity)) return MISO_E_BADARG;
  if (capacity > MISO_MESH_MAX_ENTRIES) return MISO_E_TOOLARGE;
  if (int rc = check_rays(origins, ld_o, dirs, ld_d, n, out_count)) return rc;
  return (int)launch_mesh_count_hits(*plan, workspace, lists, capacity, origins, ld_o, dirs, ld_d, n, t_min, t_max, out_count,
                                     (hipStream_t)stream);
}

int miso_mesh_count_hits_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t, int64_t n_tri,
                             const float* origins, int64_t ld_o, const float* dirs, int64_t ld_d, int64_t n, float t_min,
                             float t_max, int32_t* out_count, void* stream) {
  if (int rc = check_mesh_arrays(verts, ld_v, n_vert, tris, ld_t, n_tri)) return rc;
  if (int rc = check_rays(origins, ld_o, dirs, ld_d, n, out_count)) return rc;
  return (int)launch_mesh_count_hits_all(verts, ld_v, n_vert, tris, ld_t, n_tri, origins, ld_o, dirs, ld_d, n, t_min, t_max, out_count,
                                         (hipStream_t)stream);
}

// ---- fused atlas query (atlas.hip) ------------------------------------------------------------------------------------
int64_t miso_atlas_plan_bytes(int32_t n_submaps) {
  return n_submaps < 1 ? 0 : (int64_t)n_submaps * (int64_t)sizeof(GridK);
}

int miso_atlas_plan_build(const miso_grid_t* grids, int32_t n_submaps, void* plan_host) {
  if (!grids || !plan_host || n_submaps < 1 || n_submaps > 4096) return MISO_E_BADARG;
  GridK* out = reinterpret_cast<GridK*>(plan_host);
  for (int s = 0; s < n_submaps; ++s) {
    bool v4;
    if (int rc = convert_grid(&grids[s], &out[s], true, &v4)) return rc;
    if (!v4 || (out[s].flags & MISO_F_COORDS_NORMALIZED)) return MISO_E_UNSUPPORTED;
    if (out[s].n_levels != out[0].n_levels) return MISO_E_UNSUPPORTED;
    for (int l = 0; l < out[s].n_levels; ++l)
      if (out[s].lv[l].C != out[0].lv[0].C) return MISO_E_UNSUPPORTED;
    // (ignore_mask is the caller's: GridAtlas.query_feature passes ignore_level=None, grid_atlas.py:385 -- its grids come
    // without one; a single GridNet queried through MISO_F_ATLAS_NO_BOUND keeps its own)
  }
  return MISO_OK;
}

int miso_atlas_sdf_fwd(const void* plan, int32_t n_submaps, const miso_grid_t* shape, const float* poses,
                       const miso_mlp_t* mlp, const float* packed, const float* x, int64_t n, const float* axis_x,
                       const float* axis_y, const float* axis_z, int32_t nx, int32_t ny, int32_t nz, float* sdf,
                       float* feats, int64_t ld_feats, uint32_t flags, void* stream) {
  AtlasK a;
  if (int rc = atlas_call(&a, plan, n_submaps, poses, n, flags)) return rc;
  if (!shape || (!sdf && !feats)) return MISO_E_BADARG;
  FusedCall f;
  if (sdf) {
    if (!mlp) return MISO_E_BADARG;
    if (int rc = fused_call(&f, shape, mlp, packed, false, FUSED_ATLAS)) return rc;
  } else {      // features only: no decoder is read, the shape is still one of the kernel table's
    if (int rc = fused_grid(&f, shape, false)) return rc;
    for (int l = 0; l < f.L; ++l)
      if (f.g.lv[l].C != f.C) return MISO_E_UNSUPPORTED;
    if (!fused_shape_supported(f.C, f.L, f.H, f.NH)) return MISO_E_UNSUPPORTED;
  }
  if (feats && ld_feats < f.g.F) return MISO_E_BADARG;
  a.sdf = sdf; a.feats = feats; a.ld = ld_feats;
  if (x) {
    a.x = x;
  } else {
    if (!axis_x || !axis_y || !axis_z || nx < 1 || ny < 1 || nz < 1) return MISO_E_BADARG;
    if ((int64_t)nx * ny * nz != n || !fits32(n)) return MISO_E_BADARG;
    a.ax[0] = axis_x; a.ax[1] = axis_y; a.ax[2] = axis_z; a.dim[0] = nx; a.dim[1] = ny; a.dim[2] = nz;
  }
  return (int)launch_atlas_sdf(f.C, f.L, f.H, f.NH, a, packed, (flags & MISO_F_EXACT_F32) != 0, (hipStream_t)stream);
}

// ---- backward of the fused atlas query (atlas_bwd.hip) ------------------------------------------------------------------
int64_t miso_atlas_bwd_workspace_bytes(int64_t n, int32_t n_submaps) {
  return atlas_bwd_workspace_bytes(n, n_submaps);
}

int miso_atlas_bwd_supported(const miso_grid_t* shape, const miso_mlp_t* mlp, int32_t n_submaps, int want_poses) {
  FusedCall f;
  if (!shape || !mlp || fused_query(&f, shape, mlp, false, FUSED_ATLAS)) return 0;
  if (f.g.flags & MISO_F_COORDS_NORMALIZED) return 0;
  return atlas_bwd_covered(f.C, f.L, f.H, f.NH, n_submaps, want_poses != 0) ? 1 : 0;
}

int miso_atlas_sdf_bwd(const void* plan, int32_t n_submaps, const miso_grid_t* shape, const float* poses,
                       const miso_mlp_t* mlp, const float* packed, const float* x, int64_t n, const float* gsdf,
                       float* gx, float* gposes, void* workspace, uint32_t flags, void* stream) {
  AtlasK a;
  if (int rc = atlas_call(&a, plan, n_submaps, poses, n, flags)) return rc;
  if (!shape || !mlp) return MISO_E_BADARG;
  FusedCall f;
  if (int rc = fused_call(&f, shape, mlp, packed, false, FUSED_ATLAS)) return rc;
  if (!atlas_bwd_covered(f.C, f.L, f.H, f.NH, n_submaps, gposes != nullptr)) return MISO_E_UNSUPPORTED;
  if (n == 0) return MISO_OK;
  if (!x || !gsdf || (gposes && (!workspace || !aligned(4, workspace)))) return MISO_E_BADARG;
  a.x = x;
  return (int)launch_atlas_sdf_bwd(f.C, f.L, f.H, f.NH, a, packed, gsdf, gx, gposes, reinterpret_cast<float*>(workspace),
                                   (flags & MISO_F_EXACT_F32) != 0, (hipStream_t)stream);
}

// ---- sphere tracing through the fused atlas query (trace.hip) ------------------------------------------------------------
int miso_atlas_sphere_trace(const void* plan, int32_t n_submaps, const miso_grid_t* shape, const float* poses,
                            const miso_mlp_t* mlp, const float* packed, const float* origins, const float* dirs,
                            int64_t n_rays, float min_dist, float max_dist, int32_t max_iters, float epsilon,
                            float fd_step, float* points, uint8_t* hit, float* sdf, int32_t* steps, float* grad,
                            uint32_t flags, void* stream) {
  AtlasK a;
  if (int rc = atlas_call(&a, plan, n_submaps, poses, n_rays, flags)) return rc;
  if (!shape || !mlp || !all_set(origins, dirs, points) || !hit) return MISO_E_BADARG;
  if (max_iters < 1 || (grad && !(fd_step > 0.0f))) return MISO_E_BADARG;
  FusedCall f;
  if (int rc = fused_call(&f, shape, mlp, packed, false, FUSED_ATLAS)) return rc;
  if (n_rays == 0) return MISO_OK;
  TraceK t;
  memset(&t, 0, sizeof(t));
  t.origins = origins; t.dirs = dirs; t.n = n_rays;
  t.min_dist = min_dist; t.max_dist = max_dist; t.epsilon = epsilon; t.fd_step = fd_step; t.max_iters = max_iters;
  t.points = points; t.hit = hit; t.sdf = sdf; t.steps = steps; t.grad = grad;
  return (int)launch_atlas_trace(f.C, f.L, f.H, f.NH, a, t, packed, (flags & MISO_F_EXACT_F32) != 0, (hipStream_t)stream);
}

int64_t miso_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (mc_check_dims(nx, ny, nz)) return -1;
  return mc_workspace_bytes(nx, ny, nz);
}

int miso_mc_classify(const float* vol, int32_t nx, int32_t ny, int32_t nz, float iso, void* workspace,
                     int32_t* counts, void* stream) {
  if (int rc = mc_check_dims(nx, ny, nz)) return rc;
  if (!all_set(vol, workspace, counts) || !aligned(8, workspace)) return MISO_E_BADARG;
  return (int)launch_mc_classify(vol, nx, ny, nz, iso, workspace, counts, (hipStream_t)stream);
}

int miso_mc_emit(int32_t nx, int32_t ny, int32_t nz, void* workspace, const int64_t* offsets, int32_t n_tri_chunks,
                 int64_t capacity_tris, int64_t* faces, void* stream) {
  if (int rc = mc_check_dims(nx, ny, nz)) return rc;
  if (capacity_tris < 0 || n_tri_chunks < 0 || n_tri_chunks > mc_words(nx, ny, nz) || !workspace || !offsets ||
      (capacity_tris > 0 && !faces))
    return MISO_E_BADARG;
  return (int)launch_mc_emit(nx, ny, nz, workspace, offsets, n_tri_chunks, capacity_tris, faces, (hipStream_t)stream);
}

int miso_mc_vertices(const float* vol, int32_t nx, int32_t ny, int32_t nz, float iso, void* workspace,
                     const int64_t* offsets, int32_t n_vert_chunks, int64_t capacity_verts, float* verts,
                     void* stream) {
  if (int rc = mc_check_dims(nx, ny, nz)) return rc;
  if (capacity_verts < 0 || n_vert_chunks < 0 || n_vert_chunks > mc_words(nx, ny, nz) || !vol || !workspace ||
      !offsets || (capacity_verts > 0 && !verts))
    return MISO_E_BADARG;
  return (int)launch_mc_vertices(vol, nx, ny, nz, iso, workspace, offsets, n_vert_chunks, capacity_verts, verts,
                                 (hipStream_t)stream);
}

int miso_mc_case_table(int8_t* table_host) {
  if (!table_host) return MISO_E_BADARG;
  mc_copy_table(table_host);
  return 0;
}

}  // extern "C"
