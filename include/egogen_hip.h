/*
 * egogen_hip.h - C ABI of libegogen_hip.so: MI355X (gfx950) kernels for the EgoGen crowd_ppo hot path.
 *
 * The reference (ligengen/EgoGen) is pure Python and has no FFI layer; its de-facto operator API is a set
 * of Python call signatures.  Every entry point below names the reference call it
 * replaces (file:line relative to the reference repo root).  The Python host side (the egogen_amd Python package) binds
 * these with ctypes and mirrors the reference signatures; INTEGRATION.md shows the stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - all `const float*` / `float*` / `int*` arguments are DEVICE pointers unless the name ends in `_host`;
 *   - no entry point allocates or synchronises, except *_create / *_destroy (one-time setup);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); work is enqueued asynchronously;
 *   - return value: EGX_OK (0) or a negative error code; egx_last_error() gives a message;
 *   - fp32 everywhere; row-major; "B" = bodies (agent x frame), "A" = agents.
 */
#ifndef EGOGEN_HIP_H
#define EGOGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGX_OK 0
#define EGX_ERR_ARG (-1)
#define EGX_ERR_HIP (-2)
#define EGX_ERR_WORKSPACE (-3)
#define EGX_ERR_CONVERGENCE (-4) /* egx_geodesic_field: the pass cap was reached while the field still changed */

#define EGX_NUM_JOINTS 55      /* SMPL-X kinematic joints                */
#define EGX_NUM_JOINTS_OUT 127 /* 55 + 21 vertex joints + 51 landmarks   */
#define EGX_XB_DIM 93          /* transl3 glorot3 body63 lhand12 rhand12 */
#define EGX_MAX_CANDIDATES 256 /* candidates per sequence of egx_primitive_select */
#define EGX_MAX_BEAM 32        /* beam slots per sequence of egx_primitive_beam_select; slots * candidates <= EGX_MAX_CANDIDATES */
#define EGX_MAX_OBSTACLES 32   /* tracks per obstacle set of egx_primitive_select_obstacles: a choice, the 18-frame window of a set
                                  (18 x 32 xy and 32 radii, 4.7 KB) is staged into one workgroup's LDS */
#define EGX_MAX_GROUP 32       /* people of one group of egx_primitive_select_joint: their chosen tracks (18 x 32 xy, 4.6 KB) are one
                                  workgroup's table in LDS */
#define EGX_MAX_SWEEPS 8       /* Gauss-Seidel sweeps of egx_primitive_select_joint */
#define EGX_MAX_WAYPOINTS 16   /* waypoints of one route of egx_route_advance and egx_route_metrics */
#define EGX_MAX_LOOKAHEAD 8    /* further primitives egx_obstacle_ahead_clearance and egx_primitive_select_joint_ahead predict: the
                                  window of a set over 9 x 18 frames (41.6 KB) is staged into one workgroup's LDS */
#define EGX_GEODESIC_OFF 1.0e4f /* metres: what a geodesic field gives where none of the four surrounding cells holds a distance */
#define EGX_GEODESIC_BATCH 8    /* passes egx_geodesic_field launches between two reads of its flag */
#define EGX_NUM_BETAS 10
#define EGX_POSE_FEAT 486
#define EGX_BLEND_K 472        /* GEMM K: 10 betas + 9 x 51 movable joints = 469, padded to 8 (jaw/eyes are always identity here) */

const char* egx_last_error(void);
int egx_version(void);

/* ---------------------------------------------------------------------------------------------
 * Body model  (replaces smplx.create(...) + SMPLXParser.__init__, models/baseops.py:285-335)
 * ------------------------------------------------------------------------------------------- */
typedef struct egx_body_model egx_body_model; /* opaque; owns device copies of the packed bases */

typedef struct egx_body_model_host {
  int num_verts;                /* V (10475 for SMPL-X)                                   */
  const float* v_template_host; /* [V,3]                                                  */
  const float* shapedirs_host;  /* [V,3,10]   first 10 shape directions (expression = 0)  */
  const float* posedirs_host;   /* [486,3V]                                               */
  const float* J_regressor_host;/* [55,V]                                                 */
  const int32_t* parents_host;  /* [55], parents[0] = -1                                  */
  const float* lbs_weights_host;/* [V,55] dense; packed to ELL(nnz = max row nnz) inside  */
  const float* hand_comps_l_host; /* [12,45] */
  const float* hand_comps_r_host; /* [12,45] */
  const float* hand_mean_l_host;  /* [45]    */
  const float* hand_mean_r_host;  /* [45]    */
  const int32_t* extra_vids_host; /* [21] vertex-selected joints (smplx VertexJointSelector)   */
  const int32_t* lmk_vids_host;   /* [51,3] = faces[lmk_faces_idx]                              */
  const float* lmk_bary_host;     /* [51,3]                                                     */
  int num_markers;                /* M (67 for SSM2)                                            */
  const int32_t* marker_vids_host;/* [M]  SMPLXParser.marker (baseops.py:333-335)               */
  int num_feet;                   /* vertices excluded from penetration counting                */
  const int32_t* feet_vids_host;  /* [num_feet]  crowd_env_2f.py:53-59                          */
} egx_body_model_host;

int egx_body_model_create(const egx_body_model_host* desc, egx_body_model** out);
void egx_body_model_destroy(egx_body_model* m);
int egx_body_model_num_verts(const egx_body_model* m);
int egx_body_model_nnz(const egx_body_model* m);
/* Vertices egx_lbs_forward evaluates when no vertex output is requested: those of the 32-vertex tiles that hold a picked vertex
 * (marker, vertex joint, landmark corner) - with_sdf = 0 - or, with_sdf = 1, also a vertex of the penetration count
 * (crowd_env_2f.py:163-175 excludes the feet).  num_verts when every tile is needed.  Work accounting for bench.py. */
int egx_body_model_lbs_vertices(const egx_body_model* m, int with_sdf);

/* Scene SDF (crowd_ppo/utils.py:54-84 `sdf_dict`): grid[d0][d1][d2] indexed by the vertex (x,y,z). */
typedef struct egx_sdf_grid {
  const float* grid; /* device, [d0,d1,d2] */
  int d0, d1, d2;
  float center[3];
  float scale;
  const void* coarse_minmax; /* device table from egx_sdf_build_coarse: required by egx_lbs_forward, optional (NULL = fine grid only)
                              * elsewhere.  The table holds a bricked COPY of the grid, and that copy is what egx_sdf_sample,
                              * egx_sdf_value_grad and the egx_sdf_penalty_* calls read when this is set: the grid must not
                              * change after egx_sdf_build_coarse (rebuild the table if it does). */
} egx_sdf_grid;

/* Acceleration tables for the penetration COUNT of egx_lbs_forward: {min,max} of the fine samples each 4x4x4 block's
 * interpolation footprint can touch, followed (same buffer) by a four-level pyramid of the block maxima (free-space tests of
 * whole boxes: the work-item culling).  Trilinear interpolation is a convex combination, so a block whose bracket does not
 * contain 0 decides `calc_sdf < 0` exactly without gathering from the 64 MiB grid.  Six face tables follow the block table:
 * a point that border clamping (grid_sample padding_mode="border", utils.py:75-81) puts onto the first / last sample plane
 * of an axis only touches samples of that plane, so it is bracketed over the plane alone - bodies outside the cube are
 * decided without gathers as well.  The buffer also holds 64 auxiliary floats (the steepest slope of the interpolated field:
 * the fix-up band of blend mode 3) and a copy of the grid as 4 x 4 x 4 bricks of 256 contiguous bytes, which egx_sdf_sample
 * gathers from when the descriptor carries the table (a point's eight corners then span 2.3 cache lines instead of 4):
 * egx_sdf_coarse_bytes() is the grid's size plus ~4 %. */
size_t egx_sdf_coarse_bytes(int d0, int d1, int d2);
int egx_sdf_build_coarse(const egx_sdf_grid* sdf, void* coarse_out, void* stream);

/* Free-space culling of the work items of an SDF-counting egx_lbs_forward call (split blend modes, no vertex output): a
 * (vertex tile x 256 bodies) item all of whose bodies are provably clear of geometry for that tile - bounding box of the balls
 * around the posed joints the tile's vertices are bound to, tested against a max-pyramid of the bracket table - is skipped
 * unless the tile holds picked vertices.  Counts, joints and markers are bit-identical with and without it.  OPT-IN
 * (EGX_LBS_CULL=1 in the environment or egx_lbs_set_culling(1)): it pays when bodies stand in free space (a trained policy on a
 * learned body model: fused kernel -32 %, three small launches +0.11 ms per call at 10 240 bodies), not when they are inside
 * geometry or the model's bound is loose (profiles/r04_lbs_culling.md); egx_lbs_cull_stats reads, with a host
 * synchronisation, how many items the LAST culled call on this workspace evaluated and how many an unculled call has. */
/* 1 if SDF launches of this model are culled (convex skinning weights AND a tight bound: the blend-shape margin of the median
 * vertex tile at a reference pose is below 15 cm - learned body models; the i.i.d.-noise benchmark body is not), else 0.
 * *out_reference_margin_m (may be NULL) receives that margin in metres. */
int egx_body_model_culls(const egx_body_model* m, float* out_reference_margin_m);
int egx_lbs_set_culling(int on);
int egx_lbs_get_culling(void);
int egx_lbs_cull_stats(const egx_body_model* m, const void* workspace, int num_bodies, int32_t* out_active_items,
                       int32_t* out_total_items);

/* Bytes of scratch egx_lbs_forward needs for `num_bodies` bodies. */
/* Blend-GEMM arithmetic of egx_lbs_forward calls that do not write full vertices (process-wide switch; the environment
 * variable EGX_LBS_BLEND=f32|bf16x3|bf16x2|f16mix selects it at first use):
 *   0  fp32 MFMA (v_mfma_f32_32x32x2_f32); always used when vertices are written
 *   1  3-term bf16 split of both operands, six partial products per fp32 product on v_mfma_f32_32x32x16_bf16 with fp32
 *      accumulation: 2^-24-level accuracy (indistinguishable from mode 0) at a third of the matrix-pipe time
 *   2  2-term bf16 split, three partial products (hi.hi + hi.mid + mid.hi: 16 significant bits per operand) - and a third
 *      term for the template column, carried by a padding column of K - at a sixth of the matrix-pipe time.  The
 *      offsets it rounds are centimetres, so vertices move by <= 1.1e-6 m against the float64 oracle (mode 0: 3.7e-7) and
 *      the fused penetration counts do not change (tests/test_lbs_gpu.py::test_lbs_blend_mode_accuracy_report); all three
 *      modes are held to the same parity tolerances (north_star: 1e-4 relative).
 *   3  "f16mix" (DEFAULT): the vertex tiles that hold PICKED vertices (markers, vertex joints, landmark corners - everything the
 *      caller reads as a position) run exactly as in mode 2; the other tiles, which only feed the penetration COUNT, keep the
 *      shape / template k-steps as in mode 2 and run the 28 k-steps that hold only pose-corrective columns (centimetre-scale
 *      offsets) as ONE v_mfma_f32_32x32x16_f16 product on operands rounded to fp16 (2^-11 per operand): 204 instead of 540
 *      MFMAs per wave and work item, a third of the operand bytes.  Those vertices move by ~4e-6 m rms / ~2.2e-5 m worst case
 *      against float64 on the synthetic body (and by up to ~4e-4 m on a body built so that every rounding points the same
 *      way), so the cheap product only CLASSIFIES: a vertex whose interpolated SDF value is closer to zero than its position
 *      error can account for (a HARD bound of the blend's rounding error for that body's pose, whatever the rounding pattern,
 *      plus that of the two-plane skinning on the matrix pipe of the count-only tiles, times the steepest slope of the grid)
 *      is queued and re-evaluated in fp32 by a small kernel launched behind the fused one (vertex-major fp32 bases, the body's
 *      rotations recomputed from its parameter row, fp32 skinning) and counted from that - a few per thousand counted
 *      vertices.  The counts are those of an fp32 evaluation (crowd_env_2f.py:169-177): the parity tests hold every mode to
 *      the same 2e-5 m level-set band, and egx_lbs_fix_stats reads how many vertices the last call re-evaluated.  Positions
 *      are unaffected.
 * An unrecognised EGX_LBS_BLEND string is an error of the first egx_lbs_forward call (no silent default).
 * (No reference counterpart: smplx evaluates the blend shapes as fp32 einsum/matmul, lbs.py [upstream smplx 0.1.28].) */
int egx_lbs_set_blend_mode(int mode);
int egx_lbs_get_blend_mode(void);
/* Mode 3 only: wave tile of the fused kernel - 0 (default) = chosen by launch size: 32 vertices x 32 bodies per wave, three
 * workgroups per CU, VALU skinning, for launches of at most 20 groups of 256 bodies; 32 x 64, two workgroups per CU, count-only
 * tiles skinned on the matrix pipe, above that.  1 / 2 force one (EGX_LBS_WAVE_TILE in the environment does the same): the
 * parity tests run both on the same inputs. */
int egx_lbs_set_wave_tile(int tile);
int egx_lbs_get_wave_tile(void);
/* Mode 3 only: entries of each of the 64 sub-queues of the launch's fix-up queue that are used (0 = all 4 096).  Vertices that
 * find their sub-queue full are re-evaluated inside the fused kernel instead - slower, same result; the parity tests shrink the
 * queue to exercise that path. */
int egx_lbs_set_fix_queue_capacity(int entries);
/* Mode 3 only: vertices the last SDF-counting egx_lbs_forward call on this workspace re-evaluated in fp32 (host synchronisation). */
int egx_lbs_fix_stats(const egx_body_model* m, const void* workspace, int num_bodies, int32_t* out_reevaluated);

size_t egx_lbs_workspace_bytes(const egx_body_model* m, int num_bodies);

/*
 * egx_lbs_forward - SMPL-X forward for B bodies.
 * Replaces SMPLXParser.forward_smplx -> bm(return_verts=True, **bparam) (models/baseops.py:338-398),
 * i.e. smplx.SMPLX.forward [upstream smplx 0.1.28]: hand PCA, Rodrigues x55, shape+pose blend shapes,
 * joint regression, rigid chain, linear blend skinning, 21 vertex joints + 51 landmarks, + transl.
 * Optionally fuses the reference's follow-up on the vertices (crowd_env_2f.py:163-175): world transform
 * by the agent frame (R0,T0), calc_sdf, feet mask, per-body count of vertices with sdf < 0.
 *
 *   xb            [B,93]
 *   betas         [A,10], body b uses row b / frames_per_agent
 *   out_verts     [B,V,3]   or NULL
 *   out_joints    [B,127,3] or NULL
 *   out_markers   [B,M,3]   or NULL   (= vertices[:, marker, :])
 *   sdf           NULL = no SDF epilogue; else also needs
 *   R0 [A,3,3], T0 [A,3]    agent frames (NULL = identity), and
 *   out_pene_count [B] int32 (overwritten)
 */
int egx_lbs_forward(const egx_body_model* m, const float* xb, const float* betas, int num_bodies,
                    int frames_per_agent, float* out_verts, float* out_joints, float* out_markers,
                    const egx_sdf_grid* sdf, const float* R0, const float* T0, int32_t* out_pene_count,
                    void* workspace, size_t workspace_bytes, void* stream);

/*
 * Differentiable points - the rows of the body model at a list of vertex ids plus the 55 kinematic-tree joints, forward and
 * reverse mode: what `bm(return_verts=True, **bparam)` (models/baseops.py:382) gives under torch autograd, the gradient the
 * regressor's loss takes through the body (models_GAMMA_primitive.py:617-633).
 *
 * egx_point_set_create (models/baseops.py:382, models_GAMMA_primitive.py:617-633) gathers, once, the tables of num_points
 *   (1..1024) vertex ids from the host description egx_body_model_create takes; ids may repeat (their gradients add, as in
 *   `verts[:, vids]`); an id outside [0, V) or a count outside the range fails.  The joint regressor is folded into the
 *   template and the shape directions in float64.  destroy frees the device tables; size returns num_points.
 * egx_points_forward (models/baseops.py:382): out_points [B,P,3] = vertices[:, vids], out_joints55 [B,55,3] or NULL =
 *   joints[:, :55]; translation included, jaw and eyes at rest, betas [B / frames_per_agent, 10].
 * egx_points_backward (models_GAMMA_primitive.py:617-633 `loss.backward()`): grad_points [B,P,3] and grad_joints55 [B,55,3]
 *   (either may be NULL, not both) -> grad_xb [B,93], grad_betas_body [B,10] (one row per body; the caller sums the
 *   frames_per_agent rows of an agent).  It recomputes the forward from xb / betas: nothing is saved, there is no workspace, and
 *   no atomics are used, so the result is bit-reproducible.  batch_rodrigues [upstream smplx 0.1.28] is differentiated as
 *   written (angle = |r + 1e-8|), which is finite at the rest pose.
 */
typedef struct egx_point_set egx_point_set; /* opaque */
int egx_point_set_create(const egx_body_model_host* desc, const int32_t* vids_host, int num_points, egx_point_set** out);
void egx_point_set_destroy(egx_point_set* set);
int egx_point_set_size(const egx_point_set* set);
int egx_points_forward(const egx_point_set* set, const float* xb, const float* betas, int num_bodies, int frames_per_agent,
                       float* out_points, float* out_joints55, void* stream);
int egx_points_backward(const egx_point_set* set, const float* xb, const float* betas, int num_bodies, int frames_per_agent,
                        const float* grad_points, const float* grad_joints55, float* grad_xb, float* grad_betas_body, void* stream);

/*
 * SDF scene sets - one penetration-count launch over bodies in DIFFERENT scenes (no reference counterpart: crowd_env_2f.py trains
 * in one scene per process).  egx_sdf_scene_set_create copies, once, a device table of S records {grid, bracket table, center,
 * scale, steepest slope} from S descriptors, each with its bracket table (egx_sdf_build_coarse) and all with the same d0, d1, d2 -
 * otherwise it fails and names the scene.  It synchronises the device (the slopes are read from the tables); after it nothing is
 * allocated or copied per call, so egx_lbs_forward_scenes can be captured in a graph.  The set points at the callers' grids and
 * tables, which must outlive it; destroy frees the table only.
 */
typedef struct egx_sdf_scene_set egx_sdf_scene_set; /* opaque */
int egx_sdf_scene_set_create(const egx_sdf_grid* scenes, int num_scenes, egx_sdf_scene_set** out);
void egx_sdf_scene_set_destroy(egx_sdf_scene_set* set);
int egx_sdf_scene_set_size(const egx_sdf_scene_set* set);

/*
 * egx_lbs_forward_scenes - egx_lbs_forward with a scene per agent: body b is counted in scene agent_scene[b / frames_per_agent]
 * of `scenes` (agent_scene: device int32 [A]).  Every read of scene data - the canonical-frame -> SDF-cell map, the bracket
 * lookups, trilinear gathers and border clamp of the count, the fix-up band of blend mode 3 (that scene's slope) and the fp32
 * re-evaluation - uses the body's own scene, so each body's count, joints and markers are bit-identical to an egx_lbs_forward call
 * with that scene's descriptor on the same bodies.  All blend modes, with and without out_verts.  out_pene_count is required.
 *   An agent_scene value < 0 or >= S reads nothing outside the set: that agent's bodies get out_pene_count = -1 (their joints,
 *   markers and vertices are computed as usual).
 *   A set of one runs the one-scene kernels of egx_lbs_forward (and, after them, sets the -1 of bad indices); sets of two or more
 *   scenes run kernels that read the body's scene per body, in blend mode 3 always with the 32 x 64 wave tile
 *   (egx_lbs_set_wave_tile does not apply to them).  Free-space culling (EGX_LBS_CULL) is one-scene only: calls with a set
 *   of two or more scenes run unculled (counts are identical either way).
 */
int egx_lbs_forward_scenes(const egx_body_model* m, const float* xb, const float* betas, int num_bodies, int frames_per_agent,
                           float* out_verts, float* out_joints, float* out_markers, const egx_sdf_scene_set* scenes,
                           const int32_t* agent_scene, const float* R0, const float* T0, int32_t* out_pene_count,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * egx_lbs_joints - the 55 kinematic-tree joints of B bodies without the vertex pass: out_joints55 [B,55,3] =
 * bm(**bparam).joints[:, :55].  This is all SMPLXParser.get_new_coordinate (models/baseops.py:485: joints 0,1,2) and
 * calc_calibrate_offset (:529: joint 0 at zero global_orient / transl) take from their full SMPL-X evaluation.
 * workspace as for egx_lbs_forward.
 */
int egx_lbs_joints(const egx_body_model* m, const float* xb, const float* betas, int num_bodies, int frames_per_agent,
                   float* out_joints55, void* workspace, size_t workspace_bytes, void* stream);

/*
 * egx_canonical_frame - CanonicalCoordinateExtractor.get_new_coordinate_torch (models/baseops.py:214-225), the tail of
 * SMPLXParser.get_new_coordinate (:465-490): joints [B, joints_per_body >= 3, 3] -> out_R [B,3,3] (columns x, y, z with
 * x = normalise((j2 - j1) with z zeroed) - no epsilon, like the reference -, z = (0,0,1), y = normalise(z cross x)),
 * out_T [B,3] = joint 0 (the reference returns it as [B,1,3]).
 */
int egx_canonical_frame(const float* joints, int joints_per_body, int num_bodies, float* out_R, float* out_T, void* stream);

/*
 * egx_update_transl_glorot - SMPLXParser.update_transl_glorot, torch branch (models/baseops.py:537-598): re-express
 * transl / global_orient of xb [B,93] in the frame (R,T):  glorot' = aa(R^T aa2R(glorot))  (torchgeometry 0.1.2
 * angle_axis_to_rotation_matrix / rotation_matrix_to_angle_axis [upstream]),  transl' = R^T (transl + delta_T - T) - delta_T.
 * R [F,3,3], T [F,3] with F = num_frames in {1, B}; delta_T [B,3] = calc_calibrate_offset (:494-534) = joint 0 of
 * egx_lbs_joints at zero global_orient / transl.  out [B,93]; out == xb is the reference's inplace=True.
 */
int egx_update_transl_glorot(const float* R, const float* T, int num_frames, const float* delta_T, const float* xb, int num_bodies,
                             float* out, void* stream);

/*
 * egx_sdf_sample - calc_sdf(vertices, sdf_dict) (crowd_ppo/utils.py:54-84): trilinear, border clamp,
 * align_corners=False, negated.  pts [n,3] -> out [n].  With sdf->coarse_minmax set (egx_sdf_build_coarse) the corners are
 * gathered from the bricked copy of the grid in that buffer, otherwise from the row-major grid: bit-identical values.
 */
int egx_sdf_sample(const egx_sdf_grid* sdf, const float* pts, int64_t n, float* out, void* stream);

/*
 * egx_sdf_value_grad - calc_sdf (crowd_ppo/utils.py:54-84) with its derivative: what torch autograd gives through the
 * reference's F.grid_sample.  pts [n,3] -> out_val [n] (or NULL) = s, bit-identical to egx_sdf_sample, and out_grad [n,3] =
 * cotangent_i * g_i with g = d s / d point in value per metre (cotangent [n], NULL = 1).  Value and gradient come from the same
 * eight corners, gathered once (from the bricked copy when sdf->coarse_minmax is set, else from the row-major grid: the same
 * bits either way).  Along axis a, g_a = -(bilinear combination, with the other two axes' weights, of the four corner
 * differences along a) * scale * d_a / 2, and exactly 0 where the unclamped voxel coordinate is <= 0 or >= d_a - 1 (aten's
 * clip_coordinates_set_grad); on a cell face floor() selects the upper cell, as the value does.  This is the analytic,
 * unnormalised derivative of the returned values - not a lookup in a precomputed `gradient_grid` (the reference's commented-out
 * branch, utils.py:69-81).  n = 0 is legal.
 */
int egx_sdf_value_grad(const egx_sdf_grid* sdf, const float* pts, int64_t n, const float* cotangent, float* out_val,
                       float* out_grad, void* stream);

/*
 * egx_sdf_penalty_forward / egx_sdf_penalty_backward - a differentiable penetration penalty on arbitrary points (no reference
 * counterpart: crowd_env_2f.py:163-175 only counts).  With s_bp = calc_sdf of point p of body b:
 *   out_penalty[b] = sum_p w_p * max(margin - s_bp, 0)^power,  power in {1, 2} (2 is C1; for 1 the derivative factor is 1
 *                    where s < margin strictly, else 0);
 *   out_count[b]   = #{p : w_p > 0 and s_bp < 0}  (int32, or NULL);
 *   grad_pts[b,p]  = grad_penalty[b] * w_p * (-power * max(margin - s_bp, 0)^(power-1)) * g_bp,  g as in egx_sdf_value_grad.
 * pts [B,P,3], 1 <= P <= 2^20; weights [P] or NULL = 1.  Exactly one of sdf / scenes is non-NULL: with `scenes`, body b uses
 * scene agent_scene[b / frames_per_agent] (device int32 [B / frames_per_agent]); an index outside the set reads nothing and
 * gives penalty 0, count -1 and a zero gradient, like egx_lbs_forward_scenes.  With `sdf`, agent_scene is ignored.  The scenes
 * of a set carry their tables, so set calls always read the bricked copies; each body is bit-identical to the one-scene call.
 * The backward recomputes everything from the points: no workspace, nothing saved, no atomics.  The per-body sum is reduced in
 * a fixed order, so both directions are bit-reproducible.  The forward interpolates and sums in double (from the float32
 * samples and points): out_penalty is the float64 penalty rounded once; out_count uses the float32 value, the bits of
 * egx_sdf_sample.  The backward takes its hinge max(margin - s, 0) and the strict test s < margin from the float32 value: for a
 * point within one float32 rounding of the hinge the gradient is that of the float32 penalty, not of the reported one (for
 * power = 1 the factor is 0 or 1 there).
 */
int egx_sdf_penalty_forward(const egx_sdf_grid* sdf, const egx_sdf_scene_set* scenes, const int32_t* agent_scene, const float* pts,
                            int num_bodies, int points_per_body, int frames_per_agent, const float* weights, float margin,
                            int power, float* out_penalty, int32_t* out_count, void* stream);
int egx_sdf_penalty_backward(const egx_sdf_grid* sdf, const egx_sdf_scene_set* scenes, const int32_t* agent_scene, const float* pts,
                             int num_bodies, int points_per_body, int frames_per_agent, const float* weights, float margin,
                             int power, const float* grad_penalty, float* grad_pts, void* stream);

/*
 * egx_mesh_sdf - scene preparation (the reference ships data/room0_sdf.pkl ready-made and refers to an
 * external tool for new scenes, README.md:97): fills grid[d0][d1][d2] (indexed by x, y, z; sample (i,j,k) at
 * center + ((2i+1)/d - 1) / scale, the cell centres `calc_sdf`'s grid_sample(align_corners=False) assumes,
 * crowd_ppo/utils.py:54-84) with the signed distance to a closed triangle mesh.
 *   triangles [F,9] device (ax,ay,az,bx,by,bz,cx,cy,cz); center_host [3] host; inside_positive 1: > 0 inside the mesh
 *   (obstacle solids, the stored convention: calc_sdf negates), 0: < 0 inside (a room shell whose interior is free space).
 */
int egx_mesh_sdf(const float* triangles, int num_triangles, const float* center_host, float scale, int d0, int d1, int d2,
                 int inside_positive, float* out_grid, void* stream);

/*
 * egx_sdf_boxes - analytic scenes on the device: a room box with up to EGX_SDF_MAX_BOXES oriented boxes standing in it, in the
 * grid contract of egx_mesh_sdf (sample (i,j,k) at center + ((2i+1)/d - 1) / scale).  Replaces the host builder
 * synth.make_sdf_scene (float64 numpy, one axis-aligned box) for the reference's training distribution of random box scenes
 * (random_box_obstacle_new, environments.py:386-402).  Stored value, make_sdf_scene's convention (> 0 inside obstacles and
 * outside the room):  v = max(start, max_k(-d_k)),  d_k = exact signed distance to box k, negative inside, evaluated in the
 * box's frame (p - c rotated by -yaw about z);  start = base_grid's sample when base_grid is given (composition onto an
 * existing grid, e.g. a scan), else the signed distance to the room box.
 *   base_grid  device [d0][d1][d2] or NULL; out_grid == base_grid (in place) is allowed;
 *   room_lo_hi host [6] (lo.xyz, hi.xyz) or NULL; at least one of base_grid / room_lo_hi; base_grid wins when both are given;
 *   boxes      host [num_boxes][7]: cx, cy, half_x, half_y, z_lo, z_hi, yaw; passed to the kernel by value (no device
 *              allocation, no copy, no synchronisation); 0 <= num_boxes <= EGX_SDF_MAX_BOXES.
 */
#define EGX_SDF_MAX_BOXES 16
int egx_sdf_boxes(const float* base_grid, const float* room_lo_hi, const float* boxes, int num_boxes, const float* center_host,
                  float scale, int d0, int d1, int d2, float* out_grid, void* stream);

/*
 * egx_scan_sdf - scene preparation from a scanned room (an open, oriented triangle soup): the same grid contract as
 * egx_mesh_sdf, filled with the exact distance to the nearest triangle (nearest-triangle search through a bounding-volume
 * hierarchy) signed by the pseudo-normal of the nearest feature (Baerentzen & Aanaes 2005): < 0 on the side the normals
 * face (free space), > 0 behind the surface.  All tables come from the host builder (scene_gen.scan_sdf_tables):
 *   bvh_nodes [2^(bvh_levels+1)-1, 8] device: implicit complete binary tree in heap order (node h at row h-1, children 2h and
 *     2h+1), each row {lo.xyz, 0, hi.xyz, 0}; the leaves (depth bvh_levels) hold leaf_size consecutive triangles each;
 *   triangles [F,12] device, in leaf order: {a.xyz, degenerate, b.xyz, 0, c.xyz, 0}; a degenerate (zero-area) triangle
 *     counts for the distance but never decides a sign;
 *   pseudo_normals [F,21] device: face, edge ab / bc / ca, vertex a / b / c normals of each triangle after welding.
 */
int egx_scan_sdf(const float* bvh_nodes, int bvh_levels, const float* triangles, const float* pseudo_normals, int num_triangles,
                 int leaf_size, const float* center_host, float scale, int d0, int d1, int d2, float* out_grid, void* stream);

/*
 * egx_walkable_raster - per cell of a floor raster (cell (i,j) centred at origin + (i+0.5, j+0.5) * cell, out[i][j]):
 *   support   1 iff the centre is covered in xy by an up-facing triangle (unit normal z >= min_up_nz) whose height there is
 *             within +-floor_tol of floor_height;
 *   clearance xy distance from the centre to the footprint of the parts of the triangles inside the slab z_lo <= z <= z_hi
 *             (absolute heights; each triangle is clipped to the slab), about 1.8e19 when no triangle enters it.
 *   triangles [F,9] device (ax,ay,az,bx,by,bz,cx,cy,cz).  Free cells (erosion of the support, clearance > radius) are decided
 *   on the host (scene_gen.scan_walkable_grid).
 */
int egx_walkable_raster(const float* triangles, int num_triangles, float origin_x, float origin_y, float cell, int nx, int ny,
                        float floor_height, float floor_tol, float min_up_nz, float z_lo, float z_hi, int* out_support,
                        float* out_clearance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense layers of the rollout networks.  One fused call replaces nn.Linear + torch.cat + activation
 * (+ residual) as composed in models/baseops.py:615-641 (MLP), models_GAMMA_primitive.py:160-175
 * (ResNetBlock) and models_policy_ppo.py:24-39 (MLPBlock):   out = act(cat(x_0..x_{s-1}) W^T + b) + residual
 * ------------------------------------------------------------------------------------------- */
#define EGX_ACT_NONE 0
#define EGX_ACT_TANH 1
#define EGX_ACT_RELU 2
#define EGX_ACT_LRELU 3

typedef struct egx_linear_desc {
  int num_rows;          /* M */
  int out_features;      /* N */
  int num_segments;      /* 1..4 input segments, concatenated along the feature axis (K = sum widths) */
  const float* seg_ptr[4];
  int seg_width[4];
  int seg_ld[4];         /* row stride of each segment, in floats */
  const float* weight;   /* [N,K] torch nn.Linear layout */
  int weight_ld;         /* 0 = K */
  const float* bias;     /* [N] or NULL */
  const float* residual; /* [M,N] added AFTER the activation, or NULL */
  int residual_ld;
  float* out;            /* [M,N] */
  int out_ld;            /* 0 = N */
  int activation;        /* EGX_ACT_* */
  float leaky_slope;
} egx_linear_desc;

int egx_linear(const egx_linear_desc* d, void* stream);

/* torch.nn.GRU / GRUCell gate math given gi = x W_ih^T + b_ih and gh = h W_hh^T + b_hh ([M,3H], gate order
 * r,z,n); h_prev may be NULL (zero state).  Used for x_enc / d_rnn (models_GAMMA_primitive.py:84,94) and the
 * policy's x_enc / ego_enc (models_policy_ppo.py:291,298). */
int egx_gru_pointwise(const float* gi, const float* gh, const float* h_prev, int h_prev_ld, float* h_out,
                      int h_out_ld, int num_rows, int hidden, void* stream);

/* MoshRegressor._cont2aa (models_GAMMA_primitive.py:208-219; RotConverter.cont2aa baseops.py:143-162):
 * xb6 [n,159] (transl3 | 22x6D | hands24) -> out [n,>=93] (transl3 | 22 axis-angles | hands24). */
int egx_cont6d_to_aa(const float* xb6, int num_rows, float* out, int out_ld, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Glue of the combo training step (GAMMAPrimitiveComboTrainOP, models_GAMMA_primitive.py:713-1093).  No float atomics and a
 * fixed summation order: two calls on the same inputs give the same bits.
 *
 * egx_cont6d_to_aa_backward: reverse mode of egx_cont6d_to_aa.  xb6 [n,159], g_out [n,93] (gradient of the axis-angle row)
 *   -> g_xb6 [n,159].  The forward is recomputed from xb6 (nothing saved), per joint in double: normalise, Gram-Schmidt,
 *   normalise, cross product, the four-branch quaternion extraction on R^T, 2 atan2(|v|, w) / |v| with the w < 0 select.  The
 *   3 + 24 pass-through columns copy the incoming gradient.  At |v|^2 == 0 (an exact identity) torch's own graph of that
 *   expression yields NaN (sqrt'(0) * 0); here k = 2 is treated as a constant there and the finite value is returned.
 * egx_primitive_loss_forward (_calc_loss_rec, :773-784): Y, Y_rec [T,b,D] -> out3 = {w_rec rec + w_td td, rec, td} with
 *   rec = mean |Y - Y_rec|, td = mean |(Y_rec[1:] - Y_rec[:-1]) - (Y[1:] - Y[:-1])| (0 for T == 1).  The terms are formed in fp32
 *   as torch forms them, summed in double in an order that depends on the shape alone, and rounded once.  workspace: device
 *   buffer of EGX_PRIMITIVE_LOSS_WS_BYTES bytes, 8-byte aligned.
 * egx_primitive_loss_backward: g_Y_rec [T,b,D] = g (w_rec / N sign(Y_rec - Y) + w_td / N_td (sign(D[t-1]) - sign(D[t]))) with D the
 *   temporal-difference residual, sign(0) = 0 and g = *g_loss (a device scalar); one launch.
 * egx_primitive_reseed: the no-grad block of calc_loss_rollout (:959-984), one workgroup per sequence.  joints
 *   [b,joints_per_body,3] of the seed frame, X_prev [t_his,b,67,3], Yg [t_pred,b,67,3] (world), R_prev [b,3,3], T_prev [b,3] ->
 *   R_new, T_new: the canonical frame of the seed body (baseops.py:214-225, the arithmetic of egx_canonical_frame);
 *   R_curr = R_prev R_new; T_curr = R_prev T_new + T_prev; X = R_new^T (X_prev - T_new) [t_his,b,201];
 *   Y = R_curr^T (Yg - T_curr) [t_pred,b,201].  No gradient.
 * ------------------------------------------------------------------------------------------- */
#define EGX_PRIMITIVE_LOSS_WS_BYTES 4096
int egx_cont6d_to_aa_backward(const float* xb6, const float* g_out, int num_rows, float* g_xb6, void* stream);
int egx_primitive_loss_forward(const float* Y, const float* Y_rec, int T, int b, int D, float w_rec, float w_td, float* out3,
                               void* workspace, void* stream);
int egx_primitive_loss_backward(const float* Y, const float* Y_rec, int T, int b, int D, float w_rec, float w_td,
                                const float* g_loss, float* g_Y_rec, void* stream);
int egx_primitive_reseed(const float* joints, int joints_per_body, const float* X_prev, const float* Yg, const float* R_prev,
                         const float* T_prev, int t_his, int t_pred, int num_seqs, float* out_R_new, float* out_T_new,
                         float* out_R_curr, float* out_T_curr, float* out_X, float* out_Y, void* stream);

/* GAMMAPolicyBase.positional_encoding of obs['dist'] and obs['time'] (models_policy_ppo.py:276-285,302-303):
 * out [A,128] = [posenc(dist) 64 | posenc(time) 64]. */
int egx_posenc(const float* dist, const float* time, int num_agents, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Motion prior: GAMMAPrimitiveCombo.sample_prior(X, betas, z) (models_GAMMA_primitive.py:334-360)
 *   = GAMMAPrimitiveVAE.decode (:83-101, 18 GRUCell steps, residual)  +  MoshRegressor.forward (:262-301,
 *     3 recurrences of a 10-block ResNet, 6D -> axis-angle).
 * Weight pointers alias the torch parameters of the same state_dict keys (`predictor.*`, `regressor.*`).
 * ------------------------------------------------------------------------------------------- */
/* "Packed" matrices of the rollout dense layers (csrc/d3.h; written by csrc/pack3.hip).  The rollout networks run their products on the bf16
 * matrix pipe with every fp32 operand carried as three bf16 terms (x = hi + mid + lo, six partial products, fp32
 * accumulation: 2^-24 relative, the arithmetic of an fp32 product).  A packed image of a row-major fp32 matrix [R, K] is
 *   [2 ceil(R/32) row tiles of 16][ceil(K/32) k-steps][3 planes][64 lanes] x 8 bf16,
 *   lane l of a fragment = row (l & 15), columns 32 s + 8 (l >> 4) .. + 7   (operand order of v_mfma_f32_16x16x32_bf16),
 * zero beyond R / K.  egx_pack3 writes such an image at k-step `dst_kstep0` of a buffer that holds `dst_ksteps` k-steps per
 * row tile (a concatenated input is several images side by side in one buffer).  Weights [N, K] in torch layout are packed
 * as they are (row = output feature). */
size_t egx_pack3_bytes(int num_rows, int num_cols);
int egx_pack3(const float* src, int num_rows, int num_cols, int src_ld, int src_col0, void* dst, int dst_ksteps,
              int dst_kstep0, void* stream);

/* One dense product on fp32 row-major operands with fp32-equivalent arithmetic on the bf16 matrix pipe:
 *   out[M,N] = act(op(A) op(B)^T + bias) + res,   op(A) = A[M,K] (trans_a = 0) or A[K,M]^T (trans_a = 1),
 *                                                 op(B) = B[N,K] (trans_b = 0) or B[K,N]^T (trans_b = 1).
 * Both operands are packed into `workspace` (egx_gemm3_workspace_bytes) and multiplied by the dense kernel of the rollout
 * / update chain: two launches.  `res` may alias `out` (accumulation); `out_act` (optional) receives the activation before
 * the residual is added.  This is what the training-side autograd nodes (egogen_amd/fused_ops.py: predictor / regressor
 * training, the checker path of the PPO update) call where the reference's `loss.backward()` reaches an `nn.Linear` /
 * `nn.GRU` product: x W^T + b forward (models/baseops.py:638-641), g^T x and g W backward. */
size_t egx_gemm3_workspace_bytes(int M, int N, int K);
int egx_gemm3(const float* A, int lda, int trans_a, const float* B, int ldb, int trans_b, int M, int N, int K,
              const float* bias, int act, float slope, const float* res, int ldr, float* out, int ldo, float* out_act,
              int ldact, void* workspace, size_t workspace_bytes, void* stream);

/* Packed images of the C-VAE decoder's dense weights (all of them or none). */
typedef struct egx_prior_packed3 {
  const void *x_enc_w_ih, *x_enc_w_hh; /* [768,201], [768,256]                                  */
  const void *drnn_w[3];               /* [512,256], [256,512], [256,256]                       */
  const void *d_rnn_w_hz;              /* d_rnn_w_ih[:, 0:384]   (columns of [hx | z])           */
  const void *d_rnn_w_y;               /* d_rnn_w_ih[:, 384:585] (columns of y_p)                */
  const void *d_rnn_w_hh;              /* [768,256]                                             */
  const void *d_comb_w;                /* [768,256] (see d_comb_w below)                        */
  const void *d_mlp_w[2];              /* [512,256], [256,512]                                  */
  const void *d_out_w;                 /* [201,256]                                             */
  /* body regressor (regressor.pnet): in_fc [128,370] as its three column blocks (markers 0:201, 6D parameters 201:360,
   * betas 360:370), the 20 block layers [128,128] one after the other, out_fc [159,128]; reg_blk_b = the 20 block biases
   * as one fp32 array [20][128] */
  const void *reg_in_m, *reg_in_xb, *reg_in_betas, *reg_blk, *reg_out;
  const float* reg_blk_b;
} egx_prior_packed3;

typedef struct egx_prior_weights {
  const float *x_enc_w_ih, *x_enc_w_hh, *x_enc_b_ih, *x_enc_b_hh; /* predictor.x_enc  GRU(201,256)      */
  const float *drnn_w[3], *drnn_b[3];                             /* predictor.drnn_mlp 256-512-256-256  */
  const float *d_rnn_w_ih, *d_rnn_w_hh, *d_rnn_b_ih, *d_rnn_b_hh; /* predictor.d_rnn  GRUCell(585,256)   */
  const float *d_mlp_w[2], *d_mlp_b[2];                           /* predictor.d_mlp  256-512-256        */
  const float *d_out_w, *d_out_b;                                 /* predictor.d_out  256-201            */
  const float *reg_in_w, *reg_in_b;                               /* regressor.pnet.in_fc 370-128        */
  const float *reg_blk_w[20], *reg_blk_b[20];                     /* regressor.pnet.layers.{0..9}.layers.{0,1} */
  const float *reg_out_w, *reg_out_b;                             /* regressor.pnet.out_fc 128-159       */
  /* d_comb_w [768,256] = d_rnn_w_ih[:, 384:585] . d_out_w and d_comb_b [768] = d_rnn_w_ih[:, 384:585] . d_out_b (folded by the
   * caller, in float64).  The residual decoder feeds y_i = d_out(h_i) + y_(i-1) back into the GRU cell
   * (models_GAMMA_primitive.py:95-103), so the cell's input product obeys gi_(i+1) = gi_i + h_i . d_comb_w^T + d_comb_b: with
   * the two folded tensors the output layer leaves the 18-step critical path and is evaluated for all steps at once
   * afterwards. */
  const float *d_comb_w, *d_comb_b;
  /* Packed images (egx_pack3) of the decoder's and the regressor's weights: egx_sample_prior runs on the bf16 matrix pipe
   * (three-term splits, fp32-equivalent) with the GRU cell as one launch and the fused body regressor as another (48-row
   * workgroups, one per compute unit).  Required - the torch-layout matrices above are only read for the biases. */
  const egx_prior_packed3* packed3;
} egx_prior_weights;

size_t egx_sample_prior_workspace_bytes(int num_agents);

/*   x_hist0 / x_hist1 : the two history frames of markers, [A,201] with row stride x_ld floats
 *                       (reference passes X = states[:2, :, :201], crowd_env_2f.py:98,109)
 *   betas [A,10]; z [A,128]
 *   out_Y  [18,A,201]  predicted markers   (Y_gen)
 *   out_Yb [18,A,93]   regressed body parameters, axis-angle (Yb_gen)                               */
int egx_sample_prior(const egx_prior_weights* w, const float* x_hist0, const float* x_hist1, int x_ld,
                     const float* betas, const float* z, int num_agents, float* out_Y, float* out_Yb,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Policy networks: GAMMAPolicyBase.forward + GAMMAActor.forward + GAMMACritic.forward
 * (models_policy_ppo.py:287-306,326-330,348-350).  Pointers alias the torch parameters
 * `shared_net.*`, `actor.pnet.*`, `critic.vnet.*`.
 * ------------------------------------------------------------------------------------------- */
/* Packed images (egx_pack3) of the policy's dense weights, all of them or none; refreshed by the host after every change
 * of the parameters (once per collect during training). */
typedef struct egx_policy_packed3 {
  const void *x_enc_w_ih, *x_enc_w_hh;     /* [1536,402], [1536,512] */
  const void *ego_enc_w_ih, *ego_enc_w_hh; /* [1536,32],  [1536,512] */
  const void *actor_w[4], *actor_out_w;    /* [1152,1152] x 4, [256,1152] */
  const void *critic_w[4], *critic_out_w;  /* [1152,1152] x 4, [1,1152]   */
} egx_policy_packed3;

typedef struct egx_policy_weights {
  const float *x_enc_w_ih, *x_enc_w_hh, *x_enc_b_ih, *x_enc_b_hh;         /* shared_net.x_enc   GRU(402,512) */
  const float *ego_enc_w_ih, *ego_enc_w_hh, *ego_enc_b_ih, *ego_enc_b_hh; /* shared_net.ego_enc GRU(32,512)  */
  const float *actor_w[4], *actor_b[4];   /* actor.pnet.layers.{0,1}.layers.{0,1}  1152x1152 */
  const float *actor_out_w, *actor_out_b; /* actor.pnet.out_fc   256x1152                    */
  const float *critic_w[4], *critic_b[4]; /* critic.vnet.layers.{0,1}.layers.{0,1}           */
  const float *critic_out_w, *critic_out_b; /* critic.vnet.out_fc 1x1152                     */
  /* Packed images of the weights (egx_pack3, or the update's own: egx_policy_train_packed): egx_policy_forward runs on the
   * bf16 matrix pipe (arithmetic: egx_policy_set_precision), each GRU cell as one launch, [hx | he | posenc] assembled in
   * place.  Required. */
  const egx_policy_packed3* packed3;
} egx_policy_weights;

/* ---------------------------------------------------------------------------------------------
 * One PPO minibatch of the policy networks without autograd and without library GEMMs (csrc/update3.hip):
 * GAMMAPPOPolicy.learn's inner loop body (crowd_ppo/ppo_policy.py:189-241) - forward of shared_net / actor / critic
 * (models/models_policy_ppo.py:287-350), the clipped-PPO loss (egx_ppo_loss_packed), and the backward pass - as a fixed chain
 * of ~21 launches on the dense3 kernels.  Gradients are WRITTEN to the tensors of `egx_policy_grads` (the views of the flat
 * gradient buffer): every parameter is used once per minibatch, nothing accumulates, the buffer needs no zero fill.
 *   create   fixes the minibatch rows (a multiple of 32) and allocates every intermediate buffer;
 *   refresh  re-makes the packed images (W and W^T) of the weights: after every optimiser step;
 *   packed   hands the row-major weight images to egx_policy_forward (egx_policy_weights.packed3), so the rollout needs
 *            no packing of its own;
 *   bind     names the observation tensors of the minibatch, state [n,2,402] and egosensing [n,2,32] (fixed addresses:
 *            the gather kernel's outputs);
 *   step     runs the chain; out_terms[6] as egx_ppo_loss_packed.
 * ------------------------------------------------------------------------------------------- */
typedef struct egx_policy_grads {
  float *x_enc_w_ih, *x_enc_w_hh, *x_enc_b_ih, *x_enc_b_hh;
  float *ego_enc_w_ih, *ego_enc_w_hh, *ego_enc_b_ih, *ego_enc_b_hh;
  float *actor_w[4], *actor_b[4], *actor_out_w, *actor_out_b;
  float *critic_w[4], *critic_b[4], *critic_out_w, *critic_out_b;
} egx_policy_grads;
typedef struct egx_policy_train egx_policy_train;
int egx_policy_train_create(const egx_policy_weights* w, const egx_policy_grads* g, int num_rows, egx_policy_train** out);
void egx_policy_train_destroy(egx_policy_train* h);
int egx_policy_train_refresh(egx_policy_train* h, void* stream);
int egx_policy_train_packed(const egx_policy_train* h, egx_policy_packed3* out);
int egx_policy_train_bind(egx_policy_train* h, const float* state, const float* egosensing);
int egx_policy_train_step(egx_policy_train* h, const float* dist, const float* time, const float* act, const float* adv,
                          const float* ret, const float* logp_old, const float* adv_stats, const float* scale, float adv_eps,
                          float min_logvar, float max_logvar, float eps_clip, float vf_coef, float ent_coef, float* out_terms,
                          void* stream);
/* The same chain in two halves, for data-parallel training (no reference counterpart: the reference trains on one device).
 * `_heads` = forward, loss (ppo_policy.py:189-241) and the whole backward of the actor and critic blocks: when it has been
 * enqueued, the prefix of the flat gradient that crowd_ppo clips (actor + critic, 10.3 M of 13.2 M parameters) is final, so its
 * all-reduce can start on a side stream; `_encoders` = the backward of the two GRU encoders (the remaining 2.8 M).  Calling both
 * in order is egx_policy_train_step. */
int egx_policy_train_step_heads(egx_policy_train* h, const float* dist, const float* time, const float* act, const float* adv,
                                const float* ret, const float* logp_old, const float* adv_stats, const float* scale, float adv_eps,
                                float min_logvar, float max_logvar, float eps_clip, float vf_coef, float ent_coef, float* out_terms,
                                void* stream);
int egx_policy_train_step_encoders(egx_policy_train* h, void* stream);
/* The same minibatch behind ONE head launch.  The minibatch is named by row indices into the rollout's tensors instead of by
 * compact copies: rows idx[0..n) with idx = perm + k * n, n = the handle's rows, k = *cursor (device scalar; NULL: k = 0)
 * clamped to [0, max_cursor]; perm holds (max_cursor + 1) * n indices, each clamped to [0, num_src_rows).  In independent
 * blocks of one grid the launch writes the input images from rows idx[r] of state / egosensing, the positional encoding of
 * dist / time at idx[r], the rows idx[r] of act / adv / ret / logp_old into the compact buffers the loss kernel reads, with
 * compute_stats != 0 stats = {mean, unbiased std} of adv[idx[.]] (the bits of egx_adv_stats on the gathered rows; 0: the
 * caller wrote stats, e.g. the global moments of data-parallel training), and clears row k of `log` ([max_cursor + 1][6]),
 * where the loss kernel then accumulates the six loss terms of minibatch k.  Nothing in the chain advances the cursor:
 * egx_adamw_clip_step_cursor does, in its single-block launch, so replayed graphs need no copy between minibatches. */
typedef struct egx_update_head {
  const int64_t* perm;
  const int32_t* cursor;
  int max_cursor;
  int num_src_rows;
  const float *state, *egosensing, *dist, *time; /* [num_src_rows, 804 | 64 | 1 | 1] */
  const float *act, *adv, *ret, *logp_old;       /* [num_src_rows, 128 | 1 | 1 | 1]  */
  float *act_c, *adv_c, *ret_c, *logp_old_c;     /* [n, 128 | 1 | 1 | 1]             */
  float* stats;                                  /* [2]                              */
  int compute_stats;
  float* log;
} egx_update_head;
int egx_policy_train_head(egx_policy_train* h, const egx_update_head* head, void* stream); /* the head launch alone */
int egx_policy_train_step_cursor(egx_policy_train* h, const egx_update_head* head, const float* scale, float adv_eps,
                                 float min_logvar, float max_logvar, float eps_clip, float vf_coef, float ent_coef, void* stream);
int egx_policy_train_step_heads_cursor(egx_policy_train* h, const egx_update_head* head, const float* scale, float adv_eps,
                                       float min_logvar, float max_logvar, float eps_clip, float vf_coef, float ent_coef,
                                       void* stream);
/* Arithmetic of every product of the chain (forward, input gradients, weight gradients): 0 = each fp32 operand as three bf16
 * terms, six partial products (2^-24 relative: fp32-equivalent; default), 2 = two terms, three products (16 significant bits
 * per operand, the arithmetic of the LBS blend GEMM's default mode), 1 = operands rounded to bf16, one product ("bf16 MFMA"
 * of north_star).  fp32 accumulation, biases, activations, loss and all gradients OUTPUTS are fp32 in every mode.  Measured
 * against a float64 evaluation of crowd_ppo/ppo_policy.py:189-241 in tests/test_trainer_gpu.py (profiles/r04_p3_yardstick.txt). */
int egx_policy_train_set_precision(egx_policy_train* h, int prec);
/* How many dense-layer launches (egx_dense3_kernel) the handle's last step call enqueued: 12 for a whole minibatch, 15 with
 * EGX_UPDATE_MERGE=0 in the environment when the handle was created - the sequence before independent products of the backward
 * pass shared launches, kept as the checker of the merged one (both leave the same bits everywhere). */
int egx_policy_train_dense3_launches(const egx_policy_train* h);

/* Arithmetic of the dense layers inside egx_policy_forward (process-wide): 0 = fp32-equivalent (default; 1e-4 parity with the
 * reference's fp32 policy), 2 = operands as two bf16 terms (16 significant bits, three partial products), 1 = operands
 * rounded to bf16, products on the bf16 MFMA, fp32 accumulation - BASELINE config 5 ("main_crowd_eval ... bf16 MFMA
 * policy"), whose parity is statistical.  Gate math, biases, activations and outputs stay fp32. */
int egx_policy_set_precision(int bf16);
int egx_policy_get_precision(void);

size_t egx_policy_workspace_bytes(int num_rows);

/*   state [n,2,402], egosensing [n,2,32], dist [n], time [n]   (the obs dict, crowd_env_2f.py:311-312)
 *   out_mu [n,128], out_logvar [n,128] (unclamped, as the actor returns them), out_value [n];
 *   any output may be NULL (actor or critic branch skipped).                                          */
int egx_policy_forward(const egx_policy_weights* w, const float* state, const float* egosensing, const float* dist,
                       const float* time, int num_rows, float* out_mu, float* out_logvar, float* out_value,
                       void* workspace, size_t workspace_bytes, void* stream);

/* VPoser v1 encoder mean, eval mode (human_body_prior [upstream]; call site crowd_env_2f.py:198).
 * BatchNorm layers are folded into fc1 / fc2 by the host.  x: [n,63] with row stride x_ld -> out [n,32]. */
typedef struct egx_vposer_weights {
  const float *fc1_w, *fc1_b; /* 512x63  */
  const float *fc2_w, *fc2_b; /* 512x512 */
  const float *mu_w, *mu_b;   /* 32x512  */
  /* Packed images (egx_pack3) of fc1_w [512,63], fc2_w [512,512], mu_w [32,512]: the encoder is ONE launch on the bf16 matrix
   * pipe (three-term operands: fp32-equivalent, like the motion prior).  Required. */
  const void *fc1_w3, *fc2_w3, *mu_w3;
} egx_vposer_weights;

/* The encoder is one fused launch whose intermediates live in LDS: it needs no workspace (egx_vposer_workspace_bytes returns 0,
 * `workspace` may be NULL); the argument pair stays so that the signature matches the other network entries. */
size_t egx_vposer_workspace_bytes(int num_rows);
int egx_vposer_encode(const egx_vposer_weights* w, const float* x, int x_ld, int num_rows, float* out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Vector environment: the per-agent tail of CrowdEnv.step and CrowdEnv.reset
 * (crowd_ppo/crowd_env_2f.py:78-415, crowd_env_2f_box.py:78-440), batched over A independent agents.
 * ------------------------------------------------------------------------------------------- */
typedef struct egx_env_config {   /* cfg_samp20/MPVAEPolicy_samp_collision(_2).yaml fields used by step() */
  float reproj_factor, goal_thresh, pene_thres;
  float weight_skate, weight_floor, weight_face_target, weight_look_target, weight_success, weight_target_dist,
      weight_pene, weight_vp;
  int max_depth;
  int scene_kind;               /* 0: SDF scene (crowd_env_2f), 1: box scenes / walkability map (crowd_env_2f_box),
                                   2: dynamic crowd, boxes of the other members as holes (crowd_env_crowd_eval)    */
  int terminate_on_penetration; /* finetuning (crowd_env_2f.py:299-300) or box env (crowd_env_2f_box.py:325)       */
  int pene_type_body;           /* lossconfig.pene_type == 'body'                                                 */
  float ray_len;                /* 7 (2 when rendering), crowd_env_2f.py:556-558                                   */
  float vp_thresh;              /* mean VPoser norm of an "unrealistic pose": 11 (crowd_env_2f.py:201); 14 in
                                   crowd_env_egobody_eval.py:229.  <= 0 selects 11                                 */
  int no_goal_termination;      /* 1: only max_depth ends an episode (crowd_env_egobody_eval.py:378)               */
} egx_env_config;

typedef struct egx_env_scenes { /* static scene tables, device pointers */
  const float* edges;      /* [E,4] walkable-polygon ring edges (x0,y0,x1,y1) of all scenes, concatenated */
  const int32_t* edge_off; /* [S+1] */
  const float* tris;       /* [F,6] navmesh triangles (x0,y0,x1,y1,x2,y2), box scenes only                */
  const int32_t* tri_off;  /* [S+1] */
  const float* floor_height; /* [S] */
  const float* map_lin;    /* [map_res] = torch.linspace(-extent, extent, res)                            */
  int map_res;
  /* scene_kind 2 (main_crowd_eval.py / crowd_env_crowd_eval.py): G members per scene; walkable polygon of member k =
   * square floor [-half,half]^2 minus the world-space marker boxes of the other members ("holes", dummy_vector_env.py:34-39) */
  float* crowd_bbox;       /* [G][S][4] minx,miny,maxx,maxy; read for the others, written for member k        */
  int crowd_group;         /* G */
  int crowd_scenes;        /* S = num_agents of the call                                                    */
  int crowd_member;        /* k: which member the agents of this call are                                   */
  float crowd_floor_half;  /* 4.0 (crowd_env_crowd_eval.py:391)                                             */
  int crowd_polygon;       /* 1: exterior = ring set edges[edge_off[0]..edge_off[1]) (the walkable region of the scene's
                            * navmesh, crowd_env_egobody_eval.py:402,824) instead of the square floor               */
  int crowd_static;        /* 1: the other members' boxes are not holes (effective behaviour of
                            * crowd_env_egobody_eval.py:824 `Polygon(self.scene_poly, holes)`)            */
} egx_env_scenes;

typedef struct egx_env_state {  /* persistent per-agent state, device pointers, updated in place */
  float* state;   /* [A,2,402] canonical markers | marker->target unit vectors */
  float* seed;    /* [A,2,93]  body_param_seed                                  */
  float* R0;      /* [A,3,3]   canonical frame -> world                         */
  float* T0;      /* [A,3]                                                      */
  float* dist;    /* [A]       distance to target at the previous step          */
  int32_t* steps; /* [A]                                                        */
  float* wpath;   /* [A,2,3]   start, target (world)                            */
  int32_t* scene_idx; /* [A] or NULL (single scene); rewritten by egx_env_reset    */
} egx_env_state;

typedef struct egx_env_step_io {
  const float* Y_gen;        /* [18,A,201] from egx_sample_prior                       */
  const float* pred_params;  /* [A,20,93]  from egx_assemble_params                    */
  const float* joints;       /* [A*20,127,3] from egx_lbs_forward                      */
  const float* markers_proj; /* [A*20,67,3]                                            */
  const int32_t* pene_count; /* [A*20] (scene_kind 0) or NULL                          */
  const float* vp_emb;       /* [A*20,32] from egx_vposer_encode                       */
  const int32_t* feet_marker_idx; /* [6] main_ppo.py:298-299                           */
  float* reward;             /* [A]                                                    */
  int32_t* terminated;       /* [A]                                                    */
  float* reward_terms;       /* [A,8] skate, floor, face, look, goal, target_dist, pene, vp; or NULL */
  float* obs_ego;            /* [A,2,32] */
  float* obs_dist;           /* [A]      */
  float* obs_time;           /* [A]      */
  float* out_marker_b;       /* [A,20,67,3] blended markers (save_rollout) or NULL      */
  float* out_prev_frame;     /* [A,12] R0|T0 before the update (save_rollout) or NULL   */
  int32_t* nonfinite_count;  /* device counter or NULL: +1 per agent whose reward / target distance is not finite
                              * (the reference drops into pdb on NaN/Inf, crowd_env_2f.py:287-297; here the host polls
                              * the counter once per collect and raises) */
  int32_t* invalid_flags;    /* [A] or NULL: |= 1 when a pelvis of the 20 frames leaves the scene polygon during the first
                              * 5 steps (scene_kind 2 with crowd_polygon), |= 2 on an unrealistic pose - the two filters
                              * on which crowd_env_egobody_eval.py:208-216,229-234 abandons the sequence               */
} egx_env_step_io;

typedef struct egx_env_reset_io {
  int num_candidates;        /* K start/target candidates per agent: first accepted wins; when none passes, the last is
                              * committed and the agent is reported in out_pending (see below)             */
  const int32_t* mask;       /* [A] 1 = reset, or NULL = all                                              */
  const float* cand_pairs;   /* [A,K,2,3]                                                                 */
  const float* cand_yaw;     /* [A,K] final yaw jitter (box sampler, environments.py:528-538) or NULL     */
  const int32_t* cand_variant; /* [A,K] motion-seed variant or NULL                                        */
  const int32_t* cand_scene; /* [A,K] scene drawn with the candidate (box sampler, environments.py:376-377) or NULL */
  const int32_t* cand_valid; /* [A,K] precomputed acceptance (SDF start check) or NULL                     */
  const float* tab_joints;   /* [NV,2,127,3] motion-seed joints at identity global orient, zero transl     */
  const float* tab_markers;  /* [NV,2,67,3]                                                                */
  const float* tab_glorot;   /* [NV,2,3,3]  mocap global orient as rotation matrices                       */
  const float* tab_transl;   /* [NV,2,3]                                                                   */
  const float* tab_pose;     /* [NV,2,63]                                                                  */
  float* obs_ego;            /* [A,2,32] */
  float* obs_dist;           /* [A]      */
  float* obs_time;           /* [A]      */
  int32_t* out_choice;       /* [A] index of the committed candidate, or NULL                              */
  /* The reference draws until a start passes (`while True: ... if num_pene[0] == 0: break`, crowd_env_2f_box.py:349-416).
   * One launch tries K candidates; out_pending[a] = 1 where all K failed, 0 elsewhere (also for agents the mask skips).  The
   * caller launches again with fresh candidates and mask = out_pending (the same array may be passed as both) until its
   * retry budget is spent; on that last launch it passes forced_count, which then counts the agents that START IN
   * PENETRATION - a deviation from the reference's unbounded loop that must be observable (VecCrowdEnv.forced_accepts). */
  int32_t* out_pending;      /* [A] or NULL */
  int32_t* forced_count;     /* [1] += agents left pending by this launch, or NULL */
} egx_env_reset_io;

/* Yb = cat(seed, Yb_gen) with _blend_params (crowd_env_2f.py:117-123,729-739) -> pred_params [A,20,93] */
int egx_assemble_params(const float* seed, const float* Yb_gen, int num_agents, float* pred_params, void* stream);
/* crowd_env_2f.py:151-317 after the SMPL-X call: rewards, termination, re-canonicalisation, features, egosensing */
int egx_env_step_post(const egx_env_config* cfg, const egx_env_scenes* scenes, const egx_env_state* st,
                      const egx_env_step_io* io, int num_agents, void* stream);
/* scene sampler next_body (environments.py:65-335 / 371-627) + CrowdEnv.reset (crowd_env_2f.py:320-415) */
int egx_env_reset(const egx_env_config* cfg, const egx_env_scenes* scenes, const egx_env_state* st,
                  const egx_env_reset_io* io, int num_agents, void* stream);

/* CrowdEnv._get_feature (crowd_ppo/crowd_env_2f.py:680-727), the two outputs the environment consumes (:261-265,399,412):
 *   Y_l [nb,nt,M,3] canonical markers, pel [nb,nt,3], R0 [nb,3,3], T0 [nb,3], wpath [wpath_rows in {1,nb}, 3] (world target)
 *   out_dist_xyz [nb,nt] = clip(||R0^T (wpath - T0) - pel||, 1e-12)            (may be NULL)
 *   out_fea_marker [nb,nt,M*3] = unit vectors marker -> target (`fea_marker_3d_n`) (may be NULL)
 * The step / reset kernels evaluate the same device functions inline. */
int egx_env_get_feature(const float* Y_l, const float* pel, const float* R0, const float* T0, const float* wpath, int wpath_rows,
                        int num_bodies, int num_frames, int num_markers, float* out_dist_xyz, float* out_fea_marker, void* stream);

/* get_map (exp_GAMMAPrimitive/utils/batch_gen_amass.py:934-968) + the {1,-1} re-coding of crowd_env_2f_box.py:768-769:
 *   tris [F,3,2] navmesh triangles (xy), map_lin [res] = linspace(-extent, extent, res), R [nb,3,3], T [nb,3]
 *   out_points_scene [nb,res*res,3] (z = floor_height; may be NULL), out_local_map [nb,res*res] = 1 walkable / -1 not
 * (meshgrid with 'ij' indexing: point p = (lin[p / res], lin[p % res], 0)). */
int egx_env_get_map(const float* tris, int num_tris, float floor_height, const float* map_lin, int res, const float* R, const float* T,
                    int num_bodies, float* out_points_scene, float* out_local_map, void* stream);

/* egx_primitive_advance - the motion-only tail of CrowdEnv.step (crowd_ppo/crowd_env_2f.py:144-155, 238-265 without
 * _get_feature): the hand-off between two primitives of a chain, one workgroup per sequence, one launch, no host round trip.
 *   pred_params [B,20,93] (egx_assemble_params), Y_gen [18,B,201] (egx_sample_prior), x0 / x1: the two seed frames [B,201] with row
 *   stride x_ld floats (as egx_sample_prior takes them), joints [B*20,joints_per_body,3] with joints_per_body >= 3 (127 from
 *   egx_lbs_forward, 55 from egx_lbs_joints), markers_proj [B*20,67,3], delta_T [B,3] (calc_calibrate_offset: joint 0 at zero
 *   orientation / translation), R0 [B,3,3] / T0 [B,3]: the frame the primitive was generated in, UPDATED IN PLACE.
 *   out_marker_b [B,20,67,3] = reproj_factor * markers_proj + (1 - reproj_factor) * cat(x, Y_gen)
 *   out_pelvis [B,20,3] = joint 0;  out_R [B,3,3], out_T [B,3] = R0 / T0 before the update
 *   (R_, T_) = canonical frame of body (b, 18) from its joints 0, 1, 2 (the arithmetic of egx_canonical_frame)
 *   T0 <- R0 T_ + T0, then R0 <- R0 R_ (:247-248)
 *   out_seed_params [B,2,93] = frames 18, 19 of pred_params re-expressed in (R_, T_) (the arithmetic of egx_update_transl_glorot)
 *   out_x0 / out_x1: the next seed frames [B,201], row stride out_x_ld floats = R_^T (marker_b[:, 18:20] - T_)
 *   nonfinite [1] (may be NULL): += number of sequences with a non-finite output (the reference stops in pdb instead)
 * markers_proj and out_marker_b must be 16-byte aligned (whole records of a [K,B,20,67,3] buffer are).  No output may alias an
 * input except R0 / T0.  Row b of every output depends on row b of the inputs only. */
int egx_primitive_advance(const float* pred_params, const float* Y_gen, const float* x0, const float* x1, int x_ld,
                          const float* joints, int joints_per_body, const float* markers_proj, const float* delta_T,
                          float reproj_factor, int num_sequences, float* R0, float* T0, float* out_marker_b, float* out_pelvis,
                          float* out_R, float* out_T, float* out_seed_params, float* out_x0, float* out_x1, int out_x_ld,
                          int32_t* nonfinite, void* stream);

/* egx_primitive_select - best-of-N search over motion primitives, the scoring and the choice: one launch, one workgroup per
 * sequence.  Row r = i * num_candidates + n is candidate n of sequence i; the per-row inputs are the ones egx_primitive_advance
 * reads (Y_gen [18,rows,201], x0 / x1 with row stride x_ld, joints [rows*20,joints_per_body,3], markers_proj [rows*20,67,3]) plus
 * R0 [rows,3,3] / T0 [rows,3] (the frame the primitive was generated in, read only), pene_count [rows*20] from egx_lbs_forward (NULL:
 * no scene, the penetration term is 0 and nothing collides), goal [num_sequences,3] in world coordinates, feet_marker_idx [6] and
 * weights [5] = goal, skate, floor, pene, face (HOST memory).  On the blended markers mb = reproj_factor * markers_proj +
 * (1 - reproj_factor) * cat(x, Y_gen) (the values egx_primitive_advance writes) each term is the argument of a reward term of
 * CrowdEnv.step, never its exponential:
 *   skate = mean_{t=1..18} max(min_feet |mb[t+1] - mb[t-1]| / 2 * 40 - 0.075, 0)       (crowd_env_2f.py:181-185)
 *   floor = mean_t |min_feet (R0 mb[t] + T0).z - 0.02|                                  (:190-194)
 *   pene  = sum_t pene_count[t] / 20 / 10;  colliding = max_t pene_count[t] >= pene_thres  (:174-177)
 *   dist  = max(|R0^T (goal - T0) - joint 0 of body 19|, 1e-12)                         (:232)
 *   face  = 1 - r_face_target                                                           (:217-219)
 *   cost  = w_goal dist + w_skate skate + w_floor floor + w_pene pene + w_face face     (float32, in this order)
 * cost [rows], cost_terms [rows,5] = dist, skate, floor, pene, face, colliding [rows].  Per sequence: choice = the first row in the
 * order (all values finite before any non-finite; non-colliding before colliding; lower cost; lower index), status bit 0 = the
 * chosen row collides, bit 1 = every row held a non-finite value, reached = chosen dist < goal_thresh, goal_dist = chosen dist.
 * pred_params is not among the inputs: no term reads it.  num_candidates in [1, EGX_MAX_CANDIDATES].  No float atomics: a
 * sequence's outputs depend on its own rows only and are the same bits in any batch. */
int egx_primitive_select(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints, int joints_per_body,
                         const float* markers_proj, const float* R0, const float* T0, const int32_t* pene_count, const float* goal,
                         const int32_t* feet_marker_idx, const float* weights, float pene_thres, float goal_thresh,
                         float reproj_factor, int num_sequences, int num_candidates, int32_t* choice, int32_t* status,
                         int32_t* reached, float* goal_dist, float* cost, float* cost_terms, int32_t* colliding, void* stream);

/* egx_primitive_advance_select - egx_primitive_advance from the chosen candidate: workgroup i reads the per-row inputs (rows =
 * num_sequences * num_candidates of them) at row i * num_candidates + choice[i] (a choice outside [0, num_candidates) is clamped),
 * writes the records out_marker_b / out_pelvis / out_R / out_T and, where not NULL, out_params [num_sequences,20,93] (the chosen
 * row of pred_params) to row i of [num_sequences,...] buffers, and the next state (R0, T0 in place, out_seed_params, out_x0 /
 * out_x1) to all num_candidates rows of its group, so that every candidate of the next primitive starts from the winner
 * (crowd_env_2f.py:238-265).  The same arithmetic as egx_primitive_advance (one device function); with num_candidates = 1 and
 * choice = 0 the same bits.  nonfinite counts the sequences whose handed-on values are not finite. */
int egx_primitive_advance_select(const float* pred_params, const float* Y_gen, const float* x0, const float* x1, int x_ld,
                                 const float* joints, int joints_per_body, const float* markers_proj, const float* delta_T,
                                 float reproj_factor, int num_sequences, const int32_t* choice, int num_candidates, float* R0,
                                 float* T0, float* out_marker_b, float* out_pelvis, float* out_R, float* out_T, float* out_params,
                                 float* out_seed_params, float* out_x0, float* out_x1, int out_x_ld, int32_t* nonfinite,
                                 void* stream);

/* Beam search over motion primitives: per sequence i, beam_width (W) slots, each expanded into num_candidates (N) rows;
 * row r = (i * W + s) * N + n is candidate n of slot s.  1 <= W <= EGX_MAX_BEAM and W * N <= EGX_MAX_CANDIDATES.
 *
 * egx_primitive_beam_select - one workgroup per sequence scores its W * N rows with the row scoring of egx_primitive_select (the
 * same bits for cost [rows], cost_terms [rows,5], colliding [rows] on the same rows) and q = w_skate skate + w_floor floor + w_pene pene
 * + w_face face (the cost without its goal term, summed on its own).  acc [b,W] / ncoll [b,W]: sum of q and number of colliding nodes
 * on the path into each slot (zeros at depth 0).  Path key of a row with parent slot s = r / N: (nonfinite, ncoll[s] + colliding,
 * acc[s] + cost, r), compared lexicographically, a total order; a row with a non-finite cost, term or acc[s] + cost has
 * nonfinite = 1 and 0 for its cost in the key.  The W smallest keys go to slots 0 (best) .. W-1, per slot: beam_row (row within the
 * sequence's W * N), parent = beam_row / N, acc_out = acc[parent] + q, ncoll_out = ncoll[parent] + colliding, path_cost (the key's
 * cost), beam_status (bit 0: the node collides, bit 1: non-finite), goal_dist, reached = goal_dist < goal_thresh, all [b,W].  acc_out /
 * ncoll_out must be other buffers than acc / ncoll.  No float atomics; a sequence's outputs are the same bits in any batch. */
int egx_primitive_beam_select(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                              int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                              const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx, const float* weights,
                              float pene_thres, float goal_thresh, float reproj_factor, int num_sequences, int beam_width,
                              int num_candidates, const float* acc, const int32_t* ncoll, float* cost, float* cost_terms,
                              int32_t* colliding, int32_t* beam_row, int32_t* parent, float* acc_out, int32_t* ncoll_out,
                              float* path_cost, int32_t* beam_status, float* goal_dist, int32_t* reached, void* stream);

/* egx_primitive_advance_beam - the hand-off of egx_primitive_advance from every kept row: workgroup (i, s) reads the per-row inputs
 * at row i * W * N + beam_row[i,s] (clamped into the sequence's rows), writes the records to row (i, s) of [b,W,...] buffers
 * (out_params may be NULL) and the next state to the N rows of slot s.  Slot s' may read a row that slot s writes, so R0 / T0 are
 * read from one pair of buffers and written to another (R0_out / T0_out), as the seed frames are (x0 / x1 -> out_x0 / out_x1); the
 * caller swaps them from primitive to primitive.  A non-finite handed-on value sets bit 2 of beam_status[i,s]; there is no counter.
 * With W = 1 the same bits as egx_primitive_advance_select. */
int egx_primitive_advance_beam(const float* pred_params, const float* Y_gen, const float* x0, const float* x1, int x_ld,
                               const float* joints, int joints_per_body, const float* markers_proj, const float* delta_T,
                               float reproj_factor, int num_sequences, int beam_width, int num_candidates, const int32_t* beam_row,
                               const float* R0, const float* T0, float* R0_out, float* T0_out, float* out_marker_b,
                               float* out_pelvis, float* out_R, float* out_T, float* out_params, float* out_seed_params,
                               float* out_x0, float* out_x1, int out_x_ld, int32_t* beam_status, void* stream);

/* egx_beam_backtrack - the returned path: it ends in slot 0 of depth num_primitives - 1 and follows parent [K,b,W] back to depth 0.
 * Workgroup (k, i) copies the records of the path's slot at depth k (per slot [K,b,W,...]: beam_row, beam_status, goal_dist, reached
 * of the selection; marker_b, pelvis, R, T, params of the hand-off) into row (k, i) of the [K,b,...] outputs and writes
 * path_slot [K,b].  The marker and parameter buffers must be 16-byte aligned. */
int egx_beam_backtrack(const int32_t* parent, const int32_t* beam_row, const int32_t* beam_status, const float* goal_dist,
                       const int32_t* reached, const float* rec_marker_b, const float* rec_pelvis, const float* rec_R,
                       const float* rec_T, const float* rec_params, int num_primitives, int num_sequences, int beam_width,
                       int32_t* path_slot, int32_t* choice, int32_t* status, float* out_goal_dist, int32_t* out_reached,
                       float* out_marker_b, float* out_pelvis, float* out_R, float* out_T, float* out_params, void* stream);

/* Geodesic distance to a goal on the walkable raster (free [nx,ny] = [H,W], origin[2], cell: scene_gen.walkable_grid, the scene
 * files of scene_gen.save_scene), and the selection entries that read it as their goal term.
 *
 * egx_geodesic_field - num_fields distance fields dist [F,H,W] (metres) over the masks free_mask [num_scenes,H,W] (uint8, non-zero =
 * free); field f lies on mask field_scene[f] (NULL: mask 0, needs num_scenes == 1).  Graph: the free cells, 8 neighbours, a diagonal
 * step (di,dj) from (i,j) only where (i+di,j) and (i,j+dj) are free too; weights w1 (axis) and w2 (diagonal).  Seeds: seed_cell [n]
 * (flat f*H*W + i*W + j) with seed_value [n] (>= 0, finite); a seed outside the buffer or on a blocked cell is ignored, of two on
 * one cell the smaller holds.  Result: dist[c] = min(seed value of c, min over allowed neighbours n of dist[n] + w), one float32
 * addition per edge: float32 Dijkstra, the same bits in any order of relaxation (rounding is monotone); blocked and unreachable
 * cells hold +inf.  One launch is one pass of pull-form relaxation over 32 x 32 tiles held in LDS with a one-cell halo, iterated
 * inside the tile until it stops changing; passes read one of dist / tmp and write the other; no float atomics, no waiting
 * between workgroups.  The host launches EGX_GEODESIC_BATCH passes, then reads the flag of the last one: this entry SYNCHRONISES
 * the stream (scene set-up, not the primitive loop).  It stops at the first batch whose last pass changed nothing; after H*W + 1
 * passes (more than a shortest path has cells) it returns EGX_ERR_CONVERGENCE.  tmp [F,H,W] and flags [EGX_GEODESIC_BATCH] are
 * device workspace; *passes_host (HOST, may be NULL) receives the number of passes launched.  F*H*W < 2^31. */
int egx_geodesic_field(const uint8_t* free_mask, const int32_t* field_scene, int num_scenes, int num_fields, int H, int W, float w1,
                       float w2, const int32_t* seed_cell, const float* seed_value, int num_seeds, float* dist, float* tmp,
                       int32_t* flags, int32_t* passes_host, void* stream);

/* egx_geodesic_sample - fields dist [F,H,W] with origin [F,2] at points [F,n,2] (world xy) -> out [F,n].  u = (x - origin_x) / cell
 * - 0.5, v likewise: bilinear over the four surrounding cell centres, of which those outside the raster, holding +inf or of
 * weight 0 drop out and the rest are renormalised; EGX_GEODESIC_OFF where none is left; NaN for a NaN coordinate.  Every
 * operation rounds on its own (the device function of csrc/egx_geodesic.h, which the selection kernels call too). */
int egx_geodesic_sample(const float* dist, const float* origin, float cell, int num_fields, int H, int W, const float* points,
                        int num_points, float* out, void* stream);

/* egx_primitive_select_field / egx_primitive_beam_select_field - egx_primitive_select / egx_primitive_beam_select (the same
 * kernels, the same leading arguments) with the goal term read from a geodesic field: field_dist [num_fields,H,W], field_origin
 * [num_fields,2], field_cell, and field_index [num_sequences] (clamped into [0, num_fields); NULL: every sequence reads field 0).
 * The goal term of cost, and cost_terms[...,0], is then the field sampled (egx_geodesic_sample's function) at the world xy of the
 * last pelvis, R0 joint 0 of body 19 + T0; goal_dist and reached stay the Euclidean distance.  field_dist NULL: the entry
 * without a field, the same bits. */
int egx_primitive_select_field(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                               int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                               const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx, const float* weights,
                               float pene_thres, float goal_thresh, float reproj_factor, int num_sequences, int num_candidates,
                               int32_t* choice, int32_t* status, int32_t* reached, float* goal_dist, float* cost, float* cost_terms,
                               int32_t* colliding, const float* field_dist, const float* field_origin, float field_cell, int field_H,
                               int field_W, int num_fields, const int32_t* field_index, void* stream);
int egx_primitive_beam_select_field(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                    int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                    const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                    const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                    int num_sequences, int beam_width, int num_candidates, const float* acc, const int32_t* ncoll,
                                    float* cost, float* cost_terms, int32_t* colliding, int32_t* beam_row, int32_t* parent,
                                    float* acc_out, int32_t* ncoll_out, float* path_cost, int32_t* beam_status, float* goal_dist,
                                    int32_t* reached, const float* field_dist, const float* field_origin, float field_cell,
                                    int field_H, int field_W, int num_fields, const int32_t* field_index, void* stream);

/* egx_primitive_select_obstacles / egx_primitive_beam_select_obstacles - egx_primitive_select_field /
 * egx_primitive_beam_select_field (the same kernels, the same arguments up to field_index; field_dist may be NULL: the Euclidean
 * goal term) with moving obstacles: num_sets sets of up to max_obstacles <= EGX_MAX_OBSTACLES tracks, obs_xy
 * [num_sets,max_obstacles,num_frames,2] the world xy of each track per absolute frame (finite), obs_radius
 * [num_sets,max_obstacles] metres, obs_count [num_sets] the live tracks of each set, obs_index [num_sequences] the set of each
 * sequence (clamped into [0, num_sets); NULL: every sequence reads set 0).  A person is a vertical cylinder: z is not read.  The
 * rows of this launch are the primitive that starts at absolute frame frame0; its frames 0 and 1 are the seed every candidate
 * shares and are not scored.  Per row, over the predicted frames t = 2..19, with p_t the world xy of joint 0 of body t
 * (x = fma(R0[2], j.z, fma(R0[1], j.y, R0[0] j.x)) + T0.x, y likewise) and a_t = clamp(frame0 + t, 0, num_frames - 1) (before its
 * track an obstacle stands at its first position, after it where it stopped):
 *   c_t       = min_o sqrt((p_t.x - o.x)^2 + (p_t.y - o.y)^2) - (r_o + body_radius) over the live obstacles at frame a_t; +inf for none
 *   clearance = min_t c_t;  term = (sum_t max(0, margin - c_t)) / 18 (metres);  hit = clearance < 0
 * Every operation rounds on its own (no contraction); min is order-free; the frame sum is the fixed tree of the wave reduction
 * (lane t - 2 holds frame t, partners 32, 16, 8, 4, 2, 1 lanes up).  A NaN pelvis gives a NaN term and clearance: the row ranks as
 * non-finite and is not a hit.  cost = cost_prev + obstacle_weight * term, one rounded product and one rounded addition on what
 * the launch would have written without obstacles (the Euclidean cost, or the field's); the beam's q gains the same product, so
 * acc_out accumulates the term along the path.  colliding = the SDF collision OR hit: a hit row is in the colliding class of the
 * greedy order and a colliding node of the beam's path key; status bit 0 follows.  Outputs per row: obs_term, obs_clearance
 * (float), obs_hit (int32), [rows].  A phase of its own after the scoring and the field: the set's 18-frame window is staged into
 * LDS once per workgroup, then one wave per row.  EGX_ERR_ARG for a NULL output, max_obstacles outside [0, EGX_MAX_OBSTACLES], a NULL
 * obs_xy / obs_radius / obs_count with max_obstacles > 0, num_frames < 1, num_sets < 1, a negative or NaN margin or body_radius. */
int egx_primitive_select_obstacles(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                   int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                   const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx, const float* weights,
                                   float pene_thres, float goal_thresh, float reproj_factor, int num_sequences, int num_candidates,
                                   int32_t* choice, int32_t* status, int32_t* reached, float* goal_dist, float* cost,
                                   float* cost_terms, int32_t* colliding, const float* field_dist, const float* field_origin,
                                   float field_cell, int field_H, int field_W, int num_fields, const int32_t* field_index,
                                   const float* obs_xy, const float* obs_radius, const int32_t* obs_count, const int32_t* obs_index,
                                   int num_sets, int max_obstacles, int num_frames, int frame0, float obstacle_weight, float margin,
                                   float body_radius, float* obs_term, float* obs_clearance, int32_t* obs_hit, void* stream);
int egx_primitive_beam_select_obstacles(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                        int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                        const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                        const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                        int num_sequences, int beam_width, int num_candidates, const float* acc, const int32_t* ncoll,
                                        float* cost, float* cost_terms, int32_t* colliding, int32_t* beam_row, int32_t* parent,
                                        float* acc_out, int32_t* ncoll_out, float* path_cost, int32_t* beam_status, float* goal_dist,
                                        int32_t* reached, const float* field_dist, const float* field_origin, float field_cell,
                                        int field_H, int field_W, int num_fields, const int32_t* field_index, const float* obs_xy,
                                        const float* obs_radius, const int32_t* obs_count, const int32_t* obs_index, int num_sets,
                                        int max_obstacles, int num_frames, int frame0, float obstacle_weight, float margin,
                                        float body_radius, float* obs_term, float* obs_clearance, int32_t* obs_hit, void* stream);

/* The marker model of recorded tracks (csrc/genop_obstacle_markers.hip, the obstacle phase of csrc/genop.hip): the people of the
 * obstacle sets are their 67 world markers per absolute frame instead of cylinders, a candidate row is its own 67 blended markers in
 * the world.  Per primitive one launch of egx_obstacle_marker_clearance writes the frame clearances of every row, then
 * egx_primitive_select_obstacle_markers or egx_primitive_beam_select_obstacle_markers stands where the *_obstacles entry stands.
 *
 * egx_obstacle_marker_clearance - rows = num_sequences * rows_per_sequence (N, or W * N for a beam), row r belongs to sequence
 * g = r / rows_per_sequence; markers_proj / Y_gen / R0 / T0 as the selection of the same primitive reads them.  obs_markers
 * [num_sets,max_obstacles,num_frames,67,3] world markers of each track per absolute frame (the host sends finite values), obs_count
 * [num_sets], obs_index [num_sequences] or NULL as in egx_primitive_select_obstacles.  For row r and predicted frame f = 0..17, t = f + 2:
 *   set   = obs_index ? clamp(obs_index[g], 0, num_sets - 1) : 0;  cnt = clamp(obs_count[set], 0, min(max_obstacles, EGX_MAX_OBSTACLES))
 *   a     = clamp(frame0 + 2 + f, 0, num_frames - 1), evaluated in 64 bits
 *   m_d   = fma(rf, markers_proj[(r*20 + t)*201 + 3i + d], (1 - rf) * Y_gen[((t-2)*rows + r)*201 + 3i + d]): 1 - rf rounded, its product
 *           rounded, one fused multiply-add (the blend of egx_pair_marker_dist, every rounding stated)
 *   W_c   = fma(R0[3c+2], m_2, fma(R0[3c+1], m_1, R0[3c] * m_0)) + T0[c], c = 0, 1, 2 (the world marker of egx_pair_marker_dist)
 *   frame_clearance[r*18 + f] = sqrt(min over o < cnt and i, j < 67 of (dx^2 + dy^2) + dz^2) - skin, d. = W(r,t,i). - obs_markers[set,o,a,j].:
 *           three rounded differences, three rounded squares, the two rounded sums in that order, no contraction; the minimum is
 *           order-free; the correctly rounded root once, of the least square; one rounded subtraction.
 * +inf for an empty set.  NaN where any of the 201 world coordinates of (r, t) is not finite: the row then ranks as non-finite in
 * the selection, as a NaN pelvis does with cylinders.  A NaN obstacle coordinate drops out of the minimum (that marker is not
 * there).  One workgroup of 576 threads per row: the row's 18 x 67 world markers staged once in LDS (19.3 KB), a wave per two
 * frames, the tracks of a frame four at a time in registers.  No atomics, no waiting, nothing between workgroups.  EGX_ERR_ARG for
 * a NULL input (obs_index may be NULL) or output, num_sequences < 1, rows_per_sequence outside [1, EGX_MAX_CANDIDATES],
 * reproj_factor outside [0, 1], max_obstacles outside [0, EGX_MAX_OBSTACLES], num_frames < 1, num_sets < 1, a negative or
 * non-finite skin (NaN included). */
int egx_obstacle_marker_clearance(const float* markers_proj, const float* Y_gen, float reproj_factor, const float* R0, const float* T0,
                                  int num_sequences, int rows_per_sequence, const float* obs_markers, const int32_t* obs_count,
                                  const int32_t* obs_index, int num_sets, int max_obstacles, int num_frames, int frame0, float skin,
                                  float* frame_clearance, void* stream);

/* egx_primitive_select_obstacle_markers / egx_primitive_beam_select_obstacle_markers - egx_primitive_select_field /
 * egx_primitive_beam_select_field (the same arguments up to field_index; field_dist may be NULL) with the obstacle phase of the
 * *_obstacles entries on a table: c_t of row r and predicted frame t is frame_clearance[r*18 + t - 2] ([rows,18], as
 * egx_obstacle_marker_clearance wrote it for the rows of this launch), and everything after c_t is that phase's arithmetic and
 * order: clearance = min_t c_t; term = (sum_t max(0, margin - c_t)) / 18, one rounded difference per frame, the frame sum by the fixed
 * tree of the wave reduction (lane t - 2 holds frame t, partners 32, 16, 8, 4, 2, 1 lanes up), one rounded division; hit =
 * clearance < 0; a NaN frame makes term and clearance NaN and the row non-finite, not a hit; cost = cost_prev + obstacle_weight *
 * term, one rounded product and one rounded addition; the beam's q gains the same product; colliding = the SDF collision OR hit.
 * Kernels of their own, compile-time variants of the selection kernels: the cylinder entries run the code they ran before.
 * EGX_ERR_ARG for a NULL frame_clearance or obstacle output and a negative or NaN margin, and the *_field entries' own. */
int egx_primitive_select_obstacle_markers(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                          int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                          const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                          const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                          int num_sequences, int num_candidates, int32_t* choice, int32_t* status, int32_t* reached,
                                          float* goal_dist, float* cost, float* cost_terms, int32_t* colliding, const float* field_dist,
                                          const float* field_origin, float field_cell, int field_H, int field_W, int num_fields,
                                          const int32_t* field_index, const float* frame_clearance, float obstacle_weight, float margin,
                                          float* obs_term, float* obs_clearance, int32_t* obs_hit, void* stream);
int egx_primitive_beam_select_obstacle_markers(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                               int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                               const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                               const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                               int num_sequences, int beam_width, int num_candidates, const float* acc,
                                               const int32_t* ncoll, float* cost, float* cost_terms, int32_t* colliding,
                                               int32_t* beam_row, int32_t* parent, float* acc_out, int32_t* ncoll_out, float* path_cost,
                                               int32_t* beam_status, float* goal_dist, int32_t* reached, const float* field_dist,
                                               const float* field_origin, float field_cell, int field_H, int field_W, int num_fields,
                                               const int32_t* field_index, const float* frame_clearance, float obstacle_weight,
                                               float margin, float* obs_term, float* obs_clearance, int32_t* obs_hit, void* stream);

/* egx_primitive_select_joint - the joint step of the greedy search: the people of one scene and time line choose again against
 * each other's CURRENT choices.  One launch between a greedy selection entry (egx_primitive_select, _field or _obstacles, whose
 * cost [rows], cost_terms [rows,5], colliding [rows] it reads and whose choice / status / reached / goal_dist [num_sequences] it
 * updates) and egx_primitive_advance_select; rows = num_sequences * num_candidates, joints / R0 / T0 / goal as the selection read
 * them.  The sequences are partitioned into num_groups groups in CSR form on the device: group g holds the sequences
 * group_member[group_start[g] .. group_start[g+1]) in that order (group_start [num_groups+1], group_member [group_start[num_groups]];
 * an index is clamped into [0, num_sequences), a group's size to EGX_MAX_GROUP).  A sequence of no group is not touched in any
 * output; a sequence may be in one group only.  One workgroup per group:
 *   start   c_j = choice[j] of every member j (clamped into [0, num_candidates))
 *   table   per member j and predicted frame t = 2..19 the world xy of joint 0 of body t of row j * N + c_j,
 *           x = fma(R0[2], j.z, fma(R0[1], j.y, R0[0] j.x)) + T0.x, y likewise (the obstacle entries' nesting)
 *   sweeps  `sweeps` in [1, EGX_MAX_SWEEPS] Gauss-Seidel sweeps, all of them always, members in order.  For every row n of member i,
 *           with p_t its own world xy:
 *             c_t = min over the members j != i of sqrt((p_t.x - x_j)^2 + (p_t.y - y_j)^2) - rr,  rr = body_radius + body_radius
 *                   rounded once; +inf for a group of one.  Two rounded differences, two rounded squares, their rounded sum, the
 *                   correctly rounded root, one rounded difference, no contraction (the obstacle entries' clearance).  The min
 *                   drops a NaN distance (another member's non-finite track is not there in that frame); a NaN p_t gives NaN.
 *             pair_clearance = min_t c_t;  pair_term = (sum_t max(0, margin - c_t)) / 18, one rounded difference per frame, the frame
 *                   sum by the fixed tree of the wave reduction (lane t - 2 holds frame t, partners 32, 16, 8, 4, 2, 1 lanes up);
 *                   pair_hit = pair_clearance < 0.  A NaN frame makes term and clearance NaN, and the row is not a hit.
 *             joint_cost = cost[row] + pair_weight * pair_term, one rounded product and one rounded addition
 *             class = (finite ? 0 : 2) | colliding[row] | pair_hit, finite = cost[row], the five cost_terms of the row, pair_term
 *                   and joint_cost are all finite.  (With a field the selection also asks for a finite Euclidean distance, which
 *                   cost_terms no longer holds: such a row counts as finite here.)
 *           Member i's choice becomes the first row in the selection's order (class, joint_cost (0 where non-finite), n); column
 *           i of the table is rewritten from it before member i + 1 is visited.
 *   after the last sweep  crowd_clearance[i] = min_t c_t of member i's final track against the other members' final tracks (the
 *           same arithmetic), crowd_hit[i] = crowd_clearance[i] < 0, both [num_sequences]: did the crowd as written overlap.
 * choice is overwritten; status is rewritten: bit 0 = bit 0 of the chosen row's class, bit 1 = that class >= 2, both as evaluated
 * in the last sweep; goal_dist / reached are rewritten ONLY where the choice changed (the selection's Euclidean distance
 * arithmetic on the new row, reached = dist < goal_thresh) and keep the selection's bits elsewhere; cost, cost_terms and colliding are
 * only read.  Traces: pair_term, pair_clearance, joint_cost (float), pair_hit (int32), all [sweeps,rows], every row's values as
 * evaluated in that sweep; choice_trace [sweeps,num_sequences] the choices after each sweep; changed [sweeps,num_groups] the members
 * that changed their choice in that sweep (0: a fixed point).  A group of one keeps the selection's choice, status, goal_dist and
 * reached: its pair_term is 0.  512 threads per group, a wave per row with lanes 0..17 one frame each; no float atomics, no
 * waiting, nothing between workgroups: a group's outputs are the same bits in any batch.  EGX_ERR_ARG for a NULL output,
 * num_candidates outside [1, EGX_MAX_CANDIDATES], sweeps outside [1, EGX_MAX_SWEEPS], num_groups < 1, a negative or NaN margin or
 * body_radius, a non-finite pair_weight. */
int egx_primitive_select_joint(const float* joints, int joints_per_body, const float* R0, const float* T0, const float* goal,
                               const float* cost, const float* cost_terms, const int32_t* colliding, int num_sequences,
                               int num_candidates, const int32_t* group_start, const int32_t* group_member, int num_groups, int sweeps,
                               float pair_weight, float margin, float body_radius, float goal_thresh, int32_t* choice,
                               int32_t* status, int32_t* reached, float* goal_dist, float* pair_term, float* pair_clearance,
                               float* joint_cost, int32_t* pair_hit, int32_t* choice_trace, int32_t* changed,
                               float* crowd_clearance, int32_t* crowd_hit, void* stream);

/* Look-ahead in the primitive search (csrc/genop_obstacle_ahead.hip, csrc/genop_joint_ahead.hip): the cylinder models of the recorded
 * tracks and of the joint step see `lookahead` = H in [0, EGX_MAX_LOOKAHEAD] further primitives ahead.  The prediction rule of both:
 * with p(t) the world xy of joint 0 of body t of a row (x = fma(R0[2], j.z, fma(R0[1], j.y, R0[0] j.x)) + T0.x, y likewise: the
 * obstacle entries' nesting), a row repeats its own net displacement
 *   d      = p(19) - p(1), one rounded difference per axis (frames 18 and 19 become the next seed frames: frame t of the next
 *            primitive corresponds to this primitive's t + 18)
 *   p_h(t) = p(t) + h * d, h as a float, one rounded product and one rounded addition per axis, no contraction
 * and the clearance of predicted frame t = 2..19 is
 *   c_t    = min(c_{t,0}, min_{h=1..H} (max(0, c_{t,h}) + h * slack)), one rounded product h * slack and one rounded addition
 * where c_{t,0} is the cylinder clearance of the entry without look-ahead, same functions, same roundings, and c_{t,h} the same
 * clearance at the predicted positions.  The max means a prediction can cost but only the present can veto: a predicted overlap
 * alone never puts a row into the colliding class.  The minimum is order-free.  NaN: c_t is NaN where c_{t,0} or any c_{t,h} is
 * NaN, which the row's own coordinates alone can cause (a NaN p(t), or a NaN or infinite - infinite d from p(1) / p(19)); the test
 * for NaN comes before the max.  Everything after c_t is the existing arithmetic of the entry that reads it.
 *
 * egx_obstacle_ahead_clearance - one launch per primitive ahead of egx_primitive_select_obstacle_markers /
 * egx_primitive_beam_select_obstacle_markers, which read its table.  rows = num_sequences * rows_per_sequence (N, or W * N for a
 * beam), row r belongs to sequence g = r / rows_per_sequence; joints / R0 / T0 as the selection of the same primitive reads them; the
 * obstacle sets as egx_primitive_select_obstacles takes them (obs_index may be NULL; obs_xy / obs_radius / obs_count may be NULL with
 * max_obstacles 0).  Only the candidate is predicted - the other person's future is on record:
 *   set   = obs_index ? clamp(obs_index[g], 0, num_sets - 1) : 0;  cnt = clamp(obs_count[set], 0, min(max_obstacles, EGX_MAX_OBSTACLES))
 *   a_h   = clamp(frame0 + t + 18 h, 0, num_frames - 1), evaluated in 64 bits
 *   c_{t,h} = min_{o < cnt} sqrt((p_h(t).x - o.x)^2 + (p_h(t).y - o.y)^2) - (r_o + body_radius) over obs_xy[set, o, a_h]: r_o + body_radius
 *           rounded once, two rounded differences, two rounded squares, their rounded sum, the correctly rounded root, one rounded
 *           difference (egx_primitive_select_obstacles' c_t); +inf for an empty set; a track's NaN coordinate drops out of the minimum
 *   frame_clearance[r*18 + t - 2] = c_t
 * With lookahead 0 the table fed to the *_obstacle_markers entries gives the bits of the *_obstacles entries.  One workgroup of 512
 * threads per sequence: the set's window over the (H + 1) x 18 consecutive absolute frames staged once in LDS, a wave per row, lanes
 * 0..17 one frame each.  No atomics, no waiting, nothing between workgroups.  EGX_ERR_ARG for a NULL joints / R0 / T0 /
 * frame_clearance, a NULL obs_xy / obs_radius / obs_count with max_obstacles > 0, num_sequences < 1, joints_per_body < 1,
 * rows_per_sequence outside [1, EGX_MAX_CANDIDATES], max_obstacles outside [0, EGX_MAX_OBSTACLES], num_frames < 1, num_sets < 1,
 * lookahead outside [0, EGX_MAX_LOOKAHEAD], a negative or non-finite (NaN included) slack or body_radius, 2^31 rows or more. */
int egx_obstacle_ahead_clearance(const float* joints, int joints_per_body, const float* R0, const float* T0, int num_sequences,
                                 int rows_per_sequence, const float* obs_xy, const float* obs_radius, const int32_t* obs_count,
                                 const int32_t* obs_index, int num_sets, int max_obstacles, int num_frames, int frame0, float body_radius,
                                 int lookahead, float slack, float* frame_clearance, void* stream);

/* egx_primitive_select_joint_ahead - egx_primitive_select_joint (the same sweeps, arguments, outputs and traces; lookahead and slack
 * follow body_radius) with both people predicted: the table holds, next to every member j's 18 xy columns, the displacement d_j of its
 * CURRENT choice, rewritten with the column when the member chooses.  For row n of member i, with d its own displacement:
 *   c_{t,0} = egx_primitive_select_joint's c_t
 *   c_{t,h} = min over the members j != i of sqrt((p_h(t).x - q.x)^2 + (p_h(t).y - q.y)^2) - rr,  q = (x_j + h * d_j.x, y_j + h * d_j.y),
 *           one rounded product and one rounded addition per axis for either person, then c_{t,0}'s roundings; +inf for a group of
 *           one; another member's NaN q drops out of the minimum; a NaN p_h(t) gives NaN
 * pair_clearance is then min_t of the look-ahead c_t, pair_term its penalty, pair_hit = pair_clearance < 0 (which c_{t,0} alone can
 * cause).  crowd_clearance / crowd_hit stay at h = 0: did the crowd as written overlap.  With lookahead 0 every output is
 * egx_primitive_select_joint's, bit for bit.  EGX_ERR_ARG for what egx_primitive_select_joint rejects, lookahead outside
 * [0, EGX_MAX_LOOKAHEAD], a negative or non-finite (NaN included) slack. */
int egx_primitive_select_joint_ahead(const float* joints, int joints_per_body, const float* R0, const float* T0, const float* goal,
                                     const float* cost, const float* cost_terms, const int32_t* colliding, int num_sequences,
                                     int num_candidates, const int32_t* group_start, const int32_t* group_member, int num_groups,
                                     int sweeps, float pair_weight, float margin, float body_radius, int lookahead, float slack,
                                     float goal_thresh, int32_t* choice, int32_t* status, int32_t* reached, float* goal_dist,
                                     float* pair_term, float* pair_clearance, float* joint_cost, int32_t* pair_hit, int32_t* choice_trace,
                                     int32_t* changed, float* crowd_clearance, int32_t* crowd_hit, void* stream);

/* The marker-level pair model of the joint step (csrc/genop_joint_markers.hip): a person is the 67 blended markers of a candidate
 * row in the world, not a cylinder.  Two launches stand where egx_primitive_select_joint stands: egx_pair_marker_dist writes every
 * distance a sweep can ask for, egx_primitive_select_joint_markers runs the sweeps on that table.  Rows, groups and clamping as
 * egx_primitive_select_joint; rows = num_sequences * num_candidates (N), row r = m * N + n; everything over the predicted frames
 * t = 2..19.
 *   blended local marker a of row r at frame t, coordinate d (blend_marker of csrc/genop.hip, the same nesting: what the hand-off
 *           records):   m_d = rf * markers_proj[(r*20 + t)*201 + 3a + d] + (1 - rf) * Y_gen[((t-2)*rows + r)*201 + 3a + d]
 *                       evaluated as fma(rf, proj, (1 - rf) * pred): 1 - rf rounded, its product rounded, one fused multiply-add
 *                       (csrc/egx_markers.h, shared with egx_obstacle_marker_clearance)
 *   world marker        w_c = fma(R0[3c+2], m_2, fma(R0[3c+1], m_1, R0[3c] * m_0)) + T0[c], c = 0, 1, 2, R0 / T0 of row r
 *                       (the nesting of the pelvis of egx_primitive_select_joint, extended to z)
 *   bad row-frame       any of the 67 x 3 world coordinates of (r, t) is not finite
 *   pair distance       for rows r, r' of two different members of one group: D(r, r', t) = sqrt(min over the 67 x 67 marker pairs of
 *                       (dx^2 + dy^2) + dz^2): three rounded differences, three rounded squares, the two rounded sums in that
 *                       order, no contraction (the same bits with r and r' exchanged); the minimum is order-free; the correctly
 *                       rounded root once, of the least square.  +inf where either row-frame is bad.
 *   frame clearance     of row (i, n) against the others' current choices: c_t = (min over the members j != i of
 *                       D((i, n), (j, choice_j), t)) - pair_skin, one rounded difference; +inf for a group of one or where every
 *                       other member is bad at t; NaN where the row's own frame is bad (a group of one included).
 * Everything after c_t is egx_primitive_select_joint's arithmetic and order: pair_clearance, pair_term (the same wave tree),
 * pair_hit, joint_cost, the classes, the choice by the selection's order, all sweeps always, members in order; choice, status,
 * goal_dist and reached rewritten as there; the same traces; crowd_clearance / crowd_hit the chosen rows against the chosen rows.
 * pair_skin: markers sample the surface sparsely, so contact is declared at a marker distance below pair_skin.  body_radius is not
 * read in this model.
 *
 * egx_pair_marker_dist - pair_start [num_groups+1] (device) is the cumulative sum of P (P - 1) / 2 over the groups (the layout of
 * egx_crowd_metrics: pair q = pair_start[g] + local index of (a, b), a < b, lexicographic, a and b positions in the group),
 * num_pairs = pair_start[num_groups].  pair_dist [num_pairs,N,N,18]: entry (q, n_a, n_b, t - 2) = D(row n_a of member a, row n_b of
 * member b, t); NULL exactly where num_pairs == 0.  row_bad [rows] int32: bit t - 2 set where row-frame (r, t) is bad, written
 * for every row of the launch.  One workgroup per (pair, n_a, tile of 8 n_b): the first row's world markers stay in LDS, the
 * second member's rows stream through; a wave takes a frame, the 67 x 67 squared distances spread over its lanes; each unordered
 * pair is computed once.  A further workgroup per sequence writes row_bad.  A pair whose index pair_start does not place inside its
 * group is not written.  EGX_ERR_ARG for a NULL input or row_bad, num_candidates outside [1, EGX_MAX_CANDIDATES], num_groups < 1,
 * reproj_factor outside [0, 1] (NaN included), num_pairs < 0, pair_dist NULL with num_pairs > 0 or not NULL with num_pairs == 0. */
int egx_pair_marker_dist(const float* markers_proj, const float* Y_gen, float reproj_factor, const float* R0, const float* T0,
                         int num_sequences, int num_candidates, const int32_t* group_start, const int32_t* group_member,
                         const int32_t* pair_start, int num_groups, int num_pairs, float* pair_dist, int32_t* row_bad, void* stream);

/* egx_primitive_select_joint_markers - the sweeps on the table: pair_dist / row_bad / pair_start / num_pairs as
 * egx_pair_marker_dist wrote and took them, every other argument and output as egx_primitive_select_joint (pair_skin in the place of
 * body_radius).  One workgroup of 512 threads per group, a wave per row with lanes 0..17 one frame each; a table index past
 * num_pairs is not read (that member is not there).  No float atomics, no waiting, nothing between workgroups: a group's outputs
 * are the same bits in any batch.  EGX_ERR_ARG for a NULL input or output, num_candidates outside [1, EGX_MAX_CANDIDATES], sweeps
 * outside [1, EGX_MAX_SWEEPS], num_groups < 1, a negative or NaN margin or pair_skin, a non-finite pair_weight, num_pairs < 0,
 * pair_dist NULL with num_pairs > 0 or not NULL with num_pairs == 0. */
int egx_primitive_select_joint_markers(const float* pair_dist, const int32_t* row_bad, const int32_t* pair_start, int num_pairs,
                                       const float* joints, int joints_per_body, const float* R0, const float* T0, const float* goal,
                                       const float* cost, const float* cost_terms, const int32_t* colliding, int num_sequences,
                                       int num_candidates, const int32_t* group_start, const int32_t* group_member, int num_groups,
                                       int sweeps, float pair_weight, float margin, float pair_skin, float goal_thresh,
                                       int32_t* choice, int32_t* status, int32_t* reached, float* goal_dist, float* pair_term,
                                       float* pair_clearance, float* joint_cost, int32_t* pair_hit, int32_t* choice_trace,
                                       int32_t* changed, float* crowd_clearance, int32_t* crowd_hit, void* stream);

/* egx_primitive_observe -the observation of every sequence of the search as the env would have it after the chosen primitive
 * (crowd_ppo/crowd_env_2f.py:311-312 what step() returns; _calc_egosensing :524-613; _get_feature :680-727): the values
 * egx_env_step_post writes to state, obs_ego, obs_dist and obs_time, through the same device functions (csrc/egx_egosense.h,
 * egx_reward.h, egx_frame.h), from what a hand-off entry left on the device.  One launch ahead of egx_policy_forward.
 *   joints [rows * frames_per_row, joints 127, 3], rows = num_sequences * num_candidates; the two seed bodies of sequence i are the
 *          frames first_frame and first_frame + 1 (18 of 20 for a primitive, 0 of 2 for the start) of row i * N + c_i, c_i =
 *          choice[i] clamped into [0, num_candidates), 0 where choice is NULL
 *   R_prev [num_sequences,9] / T_prev [num_sequences,3]  the frame those joints are expressed in (the rotmat / transl record of the
 *          hand-off); R0 [rows,9] / T0 [rows,3] the new frame and x0 / x1 the new seed frames (201 values a row, row stride x_ld
 *          floats), all read at row i * N: the hand-off writes the same values to the N rows of a sequence
 *   goal [num_sequences,3] world;  edges [E,4] (x0,y0,x1,y1) / edge_off [num_scenes+1] / scene_idx [num_sequences] (clamped into
 *          [0, num_scenes)) the walkable polygons as ring edges, all three NULL for no polygon
 * Outputs, row i from sequence i's inputs alone:
 *   state [num_sequences,2,402]   per seed frame the 201 marker coordinates of x0 / x1 as they are, then for every marker the unit
 *          vector to target_l = R0^T (goal - T0) (marker_target_feature)
 *   egosensing [num_sequences,2,32]  per seed body -1 + 2 d / ray_len over 32 rays about the look-at direction, from the world
 *          positions R_prev j + T_prev of joints 23, 24, 56, 57 (egosensing_frame, float64); an eye outside the polygon reads -1 in
 *          every ray; without a polygon every ray reads +1 (the eye is inside an unbounded plane, d = ray_len)
 *   dist [num_sequences] = 1 / (d + 1), d = |R_prev^T (goal - T_prev) - joint 0 of the second seed body| clipped at 1e-12
 *          (target_to_local, target_distance);  time [num_sequences] = 1 - min(step, max_depth) / max_depth: the policy never saw a
 *          step above max_depth
 * 256 threads per sequence: wave 0 holds the 64 (frame, ray) pairs, the other waves the markers; a scene of up to 1024 edges is
 * staged in LDS once per workgroup.  No atomics, no waiting.  The outputs must not alias the inputs.  EGX_ERR_ARG for a NULL
 * argument, num_candidates outside [1, EGX_MAX_CANDIDATES], seed bodies outside a row, x_ld < 201, some but not all of the polygon
 * arrays, ray_len <= 0, step < 0, max_depth < 1. */
int egx_primitive_observe(const float* joints, int frames_per_row, int first_frame, const int32_t* choice, int num_candidates,
                          const float* R_prev, const float* T_prev, const float* R0, const float* T0, const float* x0, const float* x1,
                          int x_ld, const float* goal, const float* edges, const int32_t* edge_off, const int32_t* scene_idx,
                          int num_scenes, float ray_len, int step, int max_depth, int num_sequences, float* state, float* egosensing,
                          float* dist, float* time, void* stream);

/* egx_policy_propose - the candidate latents of every sequence from the policy's distribution (crowd_ppo/ppo_policy.py:169-178, the
 * arithmetic of egx_sample_action through the same device functions, csrc/egx_action.h).  mu / logvar [num_sequences,128] as
 * egx_policy_forward returns them (logvar unclamped), eps / z [num_sequences * num_candidates, 128]; z may be eps.  Row n of
 * sequence i:
 *   n < n_mean              z = mu[i], its bits
 *   n_mean <= n < n_policy  z = mu[i] + (temperature * exp(clamp(logvar[i], min_logvar, max_logvar))^0.5) * eps, the product in
 *                           brackets rounded once; temperature 0 gives mu[i]
 *   n >= n_policy           z = eps, bit for bit: the prior's sample
 * One thread per four values, 16-byte accesses.  EGX_ERR_ARG for a NULL or misaligned argument, num_candidates outside
 * [1, EGX_MAX_CANDIDATES], not 0 <= n_mean <= n_policy <= num_candidates, a negative or NaN temperature, min_logvar > max_logvar. */
int egx_policy_propose(const float* mu, const float* logvar, const float* eps, float min_logvar, float max_logvar, int num_sequences,
                       int num_candidates, int n_mean, int n_policy, float temperature, float* z, void* stream);

/* egx_primitive_people_boxes - what a sequence of the search publishes of itself to the people who see it: the axis-aligned world
 * xy box of the 2 x 67 markers of its two seed frames, one box for both frames (crowd_env_crowd_eval.py:345-352).  x0 / x1 / x_ld /
 * R0 / T0 / num_candidates as egx_primitive_observe reads them: 201 values at row i * num_candidates of stride x_ld, the frame at
 * row i * num_candidates.  Per marker m = (mx, my, mz), in float32:
 *   wx = fma(R0[2], mz, fma(R0[1], my, R0[0] * mx)) + T0[0], the first product rounded, two fused onto it, one rounded addition
 *   wy likewise with R0[3..5] and T0[1] (the nesting of the obstacle entries' world pelvis)
 * box [num_sequences,4] = (min wx, min wy, max wx, max wy), min / max exact and order-free (a wavefront reduction by shuffles, one
 * wave per sequence, no atomics).  A sequence one of whose 2 x 134 world coordinates is not finite gets four NaN: its box is no
 * hole for anybody.  EGX_ERR_ARG for a NULL argument, num_candidates outside [1, EGX_MAX_CANDIDATES], x_ld < 201. */
int egx_primitive_people_boxes(const float* x0, const float* x1, int x_ld, const float* R0, const float* T0, int num_candidates,
                               int num_sequences, float* box, void* stream);

/* egx_primitive_observe_people - egx_primitive_observe for a sequence that sees other people: its group-mates and its obstacle
 * tracks are holes of the walkable polygon the rays are cast against (the reference's crowd evaluation: dummy_vector_env.py:34-39,
 * 81-84 the other agents' boxes as holes, crowd_env_crowd_eval.py:796-820 egosensing against that polygon).  Every argument of
 * egx_primitive_observe up to num_sequences with its meaning, then:
 *   box [num_sequences,4]  what egx_primitive_people_boxes wrote for the same seed frames; may be NULL without groups
 *   group_start [num_groups+1] / group_member / member_group [num_sequences]  the groups of egx_primitive_select_joint in CSR form and
 *          the group of every sequence; all three NULL for no groups.  The holes of sequence i: box[m] of every member m != i of
 *          group member_group[i] (the group clamped into [0, num_groups), start, size and members as egx_primitive_select_joint
 *          clamps them, at most EGX_MAX_GROUP members); a member that has reached its goal still is one
 *   obs_xy [num_sets,max_obstacles,num_frames,2] / obs_radius / obs_count / obs_index / num_sets / max_obstacles / num_frames  the
 *          obstacles of the *_obstacles selection entries, all NULL / 0 for none; frame: the absolute frame of the first seed frame
 *          (obstacle_frame0 + 18 k).  Track o < obs_count[set] of sequence i's set (obs_index[i] clamped, set 0 where NULL; the
 *          count clamped into [0, min(max_obstacles, EGX_MAX_OBSTACLES)]) is the hole (min(ax - r, bx - r), min(ay - r, by - r),
 *          max(ax + r, bx + r), max(ay + r, by + r)), a and b its positions at the frames `frame` and `frame + 1`, each clamped into
 *          [0, num_frames) (a track is held at its first / last position), r its radius: one rounded float32 difference or sum each
 *   A box with a non-finite entry is no hole.  people_count [num_sequences] int32: the holes of the sequence, at most 31 + 32 where it
 *          is a member of its own group.
 * egosensing: the walkable region is the static polygon (even-odd over its ring edges; the unbounded plane without edges) minus
 * the UNION of the holes (shapely's union_all in the reference: a point in two overlapping boxes is in a hole).  The eye sees
 * nothing, every ray -1, where it lies outside the static polygon or in a hole (minx <= x < maxx and miny <= y < maxy).  Otherwise
 * d = the smallest hit parameter over the static edges and the four edges of every hole ((lo,lo) -> (hi,lo) -> (hi,hi) -> (lo,hi)
 * -> (lo,lo)), capped at ray_len, with the intersection test and the |end - eye| step of egosensing_frame, float64 throughout, and
 * the ray reads -1 + 2 d / ray_len (HoleEdges through egosensing_rays, csrc/egx_egosense.h).  A sequence without a hole gets the bits of
 * egx_primitive_observe; state, dist and time always do.
 * 256 threads per sequence: wave 0 stages the holes in LDS (one lane each, compacted by a ballot) and holds the 64 (frame, ray)
 * pairs, the other waves the markers; the static edges are staged as in egx_primitive_observe.  No atomics, no waiting, nothing
 * between workgroups: row i depends on sequence i's inputs, its mates' box rows and its obstacle set.  EGX_ERR_ARG for everything
 * egx_primitive_observe rejects, a NULL people_count, some but not all of the group arrays or num_groups < 1 with them, a NULL box
 * with groups, some but not all of obs_xy / obs_radius / obs_count (or num_sets < 1, or an obs_index) without them, max_obstacles
 * outside [0, EGX_MAX_OBSTACLES], num_frames < 1 with obstacles. */
int egx_primitive_observe_people(const float* joints, int frames_per_row, int first_frame, const int32_t* choice, int num_candidates,
                                 const float* R_prev, const float* T_prev, const float* R0, const float* T0, const float* x0,
                                 const float* x1, int x_ld, const float* goal, const float* edges, const int32_t* edge_off,
                                 const int32_t* scene_idx, int num_scenes, float ray_len, int step, int max_depth, int num_sequences,
                                 const float* box, const int32_t* group_start, const int32_t* group_member,
                                 const int32_t* member_group, int num_groups, const float* obs_xy, const float* obs_radius,
                                 const int32_t* obs_count, const int32_t* obs_index, int num_sets, int max_obstacles, int num_frames,
                                 int frame, int32_t* people_count, float* state, float* egosensing, float* dist, float* time,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * Measuring finished motions (csrc/motion_metrics.hip, egogen_amd/metrics.py)
 * ------------------------------------------------------------------------------------------- */
/* Columns of the two per-motion tables of egx_motion_metrics; egogen_amd/metrics.py COLUMNS holds their names and units. */
#define EGX_MM_DURATION_S 0
#define EGX_MM_SKATE_MEAN 1
#define EGX_MM_SKATE_SPEED_MEAN 2
#define EGX_MM_SKATE_SPEED_MAX 3
#define EGX_MM_FLOOR_MEAN 4
#define EGX_MM_FLOOR_MIN 5
#define EGX_MM_FLOOR_MAX 6
#define EGX_MM_CONTACT_SCORE 7
#define EGX_MM_PATH_LENGTH 8
#define EGX_MM_DISPLACEMENT 9
#define EGX_MM_SPEED_MEAN 10
#define EGX_MM_ACC_MEAN 11
#define EGX_MM_JERK_MEAN 12
#define EGX_MM_GOAL_DIST_END 13
#define EGX_MM_GOAL_DIST_MIN 14
#define EGX_MM_PENE_MEAN 15
#define EGX_MM_F64_COLS 16
#define EGX_MM_FRAMES 0
#define EGX_MM_SKATE_FRAMES 1
#define EGX_MM_FIRST_REACHED_FRAME 2
#define EGX_MM_PENE_MAX 3
#define EGX_MM_PENE_FRAMES 4
#define EGX_MM_I32_COLS 5
#define EGX_MM_FRAME_COLS 6    /* per-frame output: s, h, c, d, world pelvis x, world pelvis y */

/* The records both entries read are those of a `PrimitiveSequence` / a motion_*.pkl, float32, each primitive in its canonical
 * frame: blended_marker [num_primitives,20,67,3], pelvis_loc [num_primitives,20,3], transf_rotmat [num_primitives,3,3],
 * transf_transl [num_primitives,3]; a point m of primitive k stands at R_k m + T_k in the world.  A motion is a run of the frame
 * table: frame_src [num_frames] holds primitive * 20 + t, and motion i is its entries motion_start[i] .. motion_start[i + 1] - 1
 * (the host drops the seed frames a later primitive shares with its predecessor: 2 of a '2-frame' primitive, 1 of a '1-frame'
 * one).  motion_start is given twice: on the device for the kernel, and motion_start_host, the same [num_motions + 1] values in
 * host memory, which the entry checks before it launches; an index the kernel reads from device memory is clamped into its array.
 * All arithmetic is float64 from the float32 inputs, world transform included; no world-frame array is written.  No
 * floating-point atomics, a fixed reduction order, nothing between workgroups: a motion's and a pair's outputs are the same bits
 * run to run and in any batch.  Both are plain launches on `stream`: no host wait.
 *
 * egx_motion_metrics - one workgroup per motion.  With M_{f,k} the world positions of the six feet markers feet_marker_idx_host
 * (host memory, indices in [0, 67)), p_f the world pelvis, F the motion's frames, at 40 frames per second:
 *   s_f = 20 min_k |M_{f+1,k} - M_{f-1,k}|                  f = 1 .. F-2 (the reward's central difference, across hand-offs)
 *   h_f = min_k z(M_{f,k}) - floor_z
 *   c_f = exp(-max(|h_f| - 0.05, 0)) exp(-max(s_f - 0.075, 0))     f = 1 .. F-2
 *   d_f = max(|goal - p_f|, 1e-12) in 3-D, where goal [num_motions,3] (world, float32) is not NULL
 * out_f64 [num_motions, EGX_MM_F64_COLS]: duration_s = (F-1)/40; skate_mean = mean max(s_f - 0.075, 0); skate_speed_mean = mean
 * s_f; skate_speed_max; floor_mean = mean_f |h_f - 0.02|; floor_min / floor_max of h_f; contact_score = mean c_f; path_length =
 * sum_f |p_{f+1} - p_f|_xy; displacement = |p_{F-1} - p_0|_xy; speed_mean = path_length / duration_s; acc_mean = 1600
 * mean_{f=1..F-2} |p_{f+1} - 2 p_f + p_{f-1}|; jerk_mean = 64000 mean_{f=1..F-3} |p_{f+2} - 3 p_{f+1} + 3 p_f - p_{f-1}|;
 * goal_dist_end = d_{F-1}; goal_dist_min (NaN without goal); pene_mean = mean_f pene_count[frame_src[f]] (NaN where pene_count
 * [num_primitives*20] is NULL).  out_i32 [num_motions, EGX_MM_I32_COLS]: frames = F; skate_frames = #{s_f > 0.075};
 * first_reached_frame = the first f with d_f < goal_thresh, else -1; pene_max; pene_frames = #{count >= pene_thres} (both -1 without
 * pene_count).  out_per_frame [num_frames, EGX_MM_FRAME_COLS] or NULL: s_f, h_f, c_f, d_f, x and y of p_f; NaN where a quantity is not
 * defined.  EGX_ERR_ARG, and nothing launched, for a NULL required pointer, a motion of fewer than 4 frames, a motion_start_host that
 * decreases or leaves [0, num_frames], a feet index outside [0, 67), a negative or non-finite goal_thresh, a negative pene_thres,
 * a non-finite floor_z. */
int egx_motion_metrics(const float* blended_marker, const float* pelvis_loc, const float* transf_rotmat, const float* transf_transl,
                       int num_primitives, const int32_t* frame_src, int num_frames, const int32_t* motion_start,
                       const int32_t* motion_start_host, int num_motions, const int32_t* feet_marker_idx_host, const float* goal,
                       double goal_thresh, double floor_z, const int32_t* pene_count, int pene_thres, double* out_f64,
                       int32_t* out_i32, double* out_per_frame, void* stream);

/* egx_crowd_metrics - the people of one scene and time line: group g holds the motions group_member[group_start[g] ..
 * group_start[g + 1] - 1] (the CSR arrays of `PersonGroups`, at most EGX_MAX_GROUP members), every member starts at absolute frame
 * 0.  Pair q of the launch is, group after group, the members (a, b), a < b, of a group in lexicographic order; pair_start
 * [num_groups + 1] (device) holds the first pair of every group, group_start_host the group offsets in host memory (checked
 * before the launch), num_pairs = sum_g P_g (P_g - 1) / 2.  For every pair and absolute frame f < max_frames:
 *   clearance   [num_pairs,max_frames] = |p_a - p_b|_xy - 2 body_radius          the cylinder model of the search, in float64
 *   marker_dist [num_pairs,max_frames] = min over the 67 x 67 pairs of world markers of their distance
 * hold = 0: a pair is compared on the frames both members recorded, NaN elsewhere.  hold = 1: a member that has ended stands at
 * its last frame until the longest member of its group ends; NaN after that.  pair_list [num_pairs,2]: the two motions of every
 * pair.  One workgroup per (group, frame): the members' world markers are staged in LDS as float64 once, a wave takes a pair at a
 * time.  With num_pairs == 0 nothing is launched and EGX_OK returned.  EGX_ERR_ARG, and nothing launched, for a NULL required pointer,
 * a motion without frames, a group above EGX_MAX_GROUP, a negative or non-finite body_radius, hold outside {0, 1}, a num_pairs that is
 * not the groups' pair count, max_frames below the longest motion. */
int egx_crowd_metrics(const float* blended_marker, const float* pelvis_loc, const float* transf_rotmat, const float* transf_transl,
                      int num_primitives, const int32_t* frame_src, int num_frames, const int32_t* motion_start,
                      const int32_t* motion_start_host, int num_motions, const int32_t* group_start, const int32_t* group_member,
                      const int32_t* pair_start, const int32_t* group_start_host, int num_groups, int num_pairs, int max_frames,
                      double body_radius, int hold, double* clearance, double* marker_dist, int32_t* pair_list, void* stream);

/* egx_route_metrics - did a motion follow its route: the ordered rule of egx_route_advance (below) at frame resolution over the
 * whole motion.  waypoints [num_motions,max_waypoints,3] (world, float32, padded), count [num_motions] the live waypoints of each
 * motion (clamped into [0, max_waypoints]; 0: the motion has no route).  With h_f(j) = |p_f - w_j|_xy in float64 and s_0 = 0,
 * s_j = pass_frame[j-1]:
 *   pass_frame   [num_motions,max_waypoints] = the first f >= s_j with h_f(j) < pass_radius for j < count - 1 where j - 1 was passed
 *                (the next waypoint may be passed at that same frame), else -1; the last waypoint is arrived at, never passed: -1
 *   approach_min [num_motions,max_waypoints] = min_{f >= s_j} h_f(j) for j < count where j - 1 was passed, else NaN
 *   waypoints_passed [num_motions] = #{j : pass_frame[j] >= 0}
 * One workgroup per motion; the minima do not depend on an order.  EGX_ERR_ARG, and nothing launched, for a NULL pointer, a motion
 * without frames, max_waypoints outside [1, EGX_MAX_WAYPOINTS], a negative or non-finite pass_radius. */
int egx_route_metrics(const float* blended_marker, const float* pelvis_loc, const float* transf_rotmat, const float* transf_transl,
                      int num_primitives, const int32_t* frame_src, int num_frames, const int32_t* motion_start,
                      const int32_t* motion_start_host, int num_motions, const float* waypoints, const int32_t* count,
                      int max_waypoints, double pass_radius, int32_t* pass_frame, double* approach_min, int32_t* waypoints_passed,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Waypoint routes of the primitive search (csrc/genop_route.hip, egogen_amd/route.py)
 * ------------------------------------------------------------------------------------------- */
/* egx_route_advance - one launch per primitive of `generate_sequence_to_goal(route=)`, after egx_primitive_advance_select: moves the
 * cursor of every sequence along its route and rewrites the live goal (and field index) every kernel of the next primitive reads.
 * It reads only what the hand-off recorded for the primitive: pelvis_loc [b,20,3], transf_rotmat [b,3,3], transf_transl [b,3]; and
 * waypoints [b,max_waypoints,3] (world, padded), count [b] (clamped into [1, max_waypoints]), cursor [b] (clamped into
 * [0, count - 1]), field_of [b,max_waypoints] (the field of every waypoint; read only with field_index).  For sequence g with
 * cursor c, count n, waypoints w, in float32 with one rounding per operation:
 *   x_f = fma(R2, p2, fma(R1, p1, R0 * p0)) + T0, y_f likewise with row 1 of R, for the predicted frames f = 2 .. 19
 *   h(f, j) = sqrt(dx * dx + dy * dy), dx = x_f - w_j.x, dy = y_f - w_j.y
 *   route_goal[g] = w[c] and route_pass_dist[g] = min_f h(f, c), both before the update
 *   cascade: f0 = 2; while c < n - 1: the first f in [f0, 19] with h(f, c) < pass_radius; none: stop; else c += 1, f0 = f (the
 *   next waypoint may be passed at that same frame).  The last waypoint is never passed.
 * A NaN in any of the 18 positions: the cursor stays and route_pass_dist is NaN.  Written: cursor[g] and route_cursor[g] (the cursor
 * after the primitive), goal[g] = w[c] (bitwise), field_index[g] = field_of[g][c] where field_index is not NULL, and reached[g] = 0
 * unless the cursor before the update stood on the last waypoint (the selection wrote that flag against an intermediate point).
 * One wave per sequence, a frame per lane; the first frame is a ballot and the distance a minimum, neither depends on an order; no
 * atomics.  A plain launch on `stream`.  EGX_ERR_ARG for a NULL pointer (field_of and field_index may be NULL; field_index needs
 * field_of), num_sequences < 1, max_waypoints outside [1, EGX_MAX_WAYPOINTS], a negative or NaN pass_radius. */
int egx_route_advance(const float* pelvis_loc, const float* transf_rotmat, const float* transf_transl, const float* waypoints,
                      const int32_t* count, const int32_t* field_of, int num_sequences, int max_waypoints, float pass_radius,
                      int32_t* cursor, float* goal, int32_t* field_index, int32_t* reached, int32_t* route_cursor, float* route_goal,
                      float* route_pass_dist, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PPO rollout glue
 * ------------------------------------------------------------------------------------------- */
/* GAMMAPPOPolicy.forward tail (crowd_ppo/ppo_policy.py:169-178): logvar is clamped IN PLACE to [min,max];
 * act = mu + exp(logvar)^0.5 * eps (eps ~ N(0,1) supplied by the caller; ignored when deterministic != 0, the
 * `deterministic_eval and not training` branch); logp [n] (may be NULL) = Independent(Normal,1).log_prob(act). */
int egx_sample_action(const float* mu, float* logvar, const float* eps, float min_logvar, float max_logvar,
                      int deterministic, int num_rows, float* act, float* logp, void* stream);

/* GAE of process_fn/_compute_returns (crowd_ppo/ppo_policy.py:105-140; tianshou compute_episodic_return [upstream]):
 * values [n+1,A] = critic on obs_0..obs_n, rew/terminated [n,A] time-major -> returns, adv [n,A]. */
int egx_gae(const float* values, const float* rew, const int32_t* terminated, int num_steps, int num_agents,
            double gamma, double gae_lambda, float* returns, float* adv, void* stream);

/* Profiling hook for bench.py: the next egx_lbs_forward on this host thread records `start`/`stop`
 * (hipEvent_t passed as void*) immediately around its fused blend+skinning kernel launch. */
int egx_profile_next_lbs(void* start_event, void* stop_event);
int egx_event_create(void** out_event);
int egx_event_destroy(void* event);
int egx_event_elapsed_ms(void* start_event, void* stop_event, float* out_ms); /* synchronises on stop_event */


/* ---------------------------------------------------------------------------------------------
 * PPO update: fused loss + gradient of one minibatch (crowd_ppo/ppo_policy.py:189-241) and the backward of the
 * GRU gate math.  Used inside egx_policy_train_step and as custom autograd nodes by the host (whose products are egx_gemm3).
 *   loss = scale * sum_rows [ -min(r A, clamp(r,1-e,1+e) A) + vf_coef (ret - V)^2 - ent_coef H ],  r = exp(logp - logp_old),
 *   A = (adv - adv_stats[0]) / (adv_stats[1] + adv_eps) when adv_stats != NULL (per-minibatch normalisation, :192-195)
 *   logvar is the RAW actor output; the clamp to [min,max] (ppo_policy.py:169) and its gradient mask are applied inside.
 *   out_terms[6] = loss, loss/clip, loss/vf, loss/ent, loss/kld, mean(logp_old - logp)   (each x scale)
 * ------------------------------------------------------------------------------------------- */
int egx_ppo_loss(const float* mu, const float* logvar, const float* value, const float* act, const float* adv,
                 const float* ret, const float* logp_old, const float* adv_stats, const float* scale, float adv_eps,
                 float min_logvar, float max_logvar, float eps_clip, float vf_coef, float ent_coef, int num_rows,
                 float* g_mu, float* g_logvar, float* g_value, float* out_terms, void* stream);
/* The same on the actor head's raw output zp [n,256] = [mu | logvar] (models_policy_ppo.py:313-317 splits it after the fact):
 * no split / re-join copies on the way in, one gradient tensor g_zp [n,256] on the way out. */
int egx_ppo_loss_packed(const float* zp, const float* value, const float* act, const float* adv, const float* ret,
                        const float* logp_old, const float* adv_stats, const float* scale, float adv_eps, float min_logvar,
                        float max_logvar, float eps_clip, float vf_coef, float ent_coef, int num_rows, float* g_zp, float* g_value,
                        float* out_terms, void* stream);

/* Backward of egx_gru_pointwise: (gi, gh, h_prev, dh) -> d gi, d gh [M,3H], d h_prev [M,H] (NULL to skip).
 * Tensors are dense (row strides H / 3H). */
int egx_gru_pointwise_bwd(const float* gi, const float* gh, const float* h_prev, const float* dh, int num_rows, int hidden,
                          float* dgi, float* dgh, float* dh_prev, void* stream);

/* Dense-layer glue of the PPO update (GAMMAPPOPolicy.learn, crowd_ppo/ppo_policy.py:182-265: loss.backward() through
 * nn.Linear + activation (+ residual) of models_policy_ppo.py:24-39,233-274).  The matrix products are library GEMMs;
 * these two kernels replace the activation / residual / activation-gradient / bias-gradient element-wise passes.
 * activation codes as in egx_linear_desc.  egx_act_fwd: z [M,N] <- act(z) in place; out <- act(z) + res when res != NULL.
 * egx_act_bwd_colsum: g <- dy * act'(a) (a = saved activation output; g may be NULL) and db_accum[n] += sum_m g[m][n]
 * (db_accum may be NULL). */
int egx_act_fwd(float* z, const float* res, float* out, int num_rows, int width, int act, float slope, void* stream);
int egx_act_bwd_colsum(const float* dy, const float* a, float* g, float* db_accum, int num_rows, int width, int act,
                       float slope, void* stream);

/* Minibatch assembly of GAMMAPPOPolicy.learn (ppo_policy.py:189-193: `for minibatch in batch.split(...)`, tianshou
 * Batch indexing [upstream]): dst[t][r, :] = src[t][idx[r], :] for up to 8 dense row-major fp32 tensors in one launch.
 * src / width / dst are HOST arrays of device pointers / row widths. */
int egx_gather_rows(const int64_t* idx, int num_rows, int num_tensors, const float* const* src, const int* width,
                    float* const* dst, void* stream);

/* Advantage normalisation statistics of one minibatch (ppo_policy.py:195-197): out = {mean, unbiased std}. */
int egx_adv_stats(const float* adv, int n, float* out_mean_std, void* stream);

/* Episode statistics of the training collector (tianshou Collector.collect [upstream], crowd_ppo/main_ppo.py:177-183):
 * ep_ret += rew, ep_len += 1; for finished agents the totals are added to done_sums = {sum of returns, sum of lengths,
 * episode count} and the running values reset. */
int egx_track_episode(const float* rew, const int32_t* term, int num_agents, float* ep_ret, float* ep_len, float* done_sums,
                      void* stream);
/* The same bookkeeping fused with the collector's per-step stores (tianshou Collector.collect [upstream] -> ReplayBuffer.add,
 * main_ppo.py:177-183): obs (state [A,2,402], egosensing [A,2,32], dist [A], time [A]) -> rollout slot t+1, reward / terminated
 * -> slot t.  rew_dst / term_dst / ep_ret may be NULL (the first observation of a collect has no reward yet). */
int egx_rollout_store(const float* state, const float* egosensing, const float* dist, const float* time, const float* rew,
                      const int32_t* term, int num_agents, float* state_dst, float* ego_dst, float* dist_dst, float* time_dst,
                      float* rew_dst, int32_t* term_dst, float* ep_ret, float* ep_len, float* done_sums, void* stream);

/* One optimiser step of GAMMAPPOPolicy.learn (ppo_policy.py:243-247: clip_grad_norm_ over the actor+critic parameters,
 * optim.step() with the AdamW of main_ppo.py:134) over FLAT fp32 buffers of n elements: the gradient norm of the first
 * n_clip elements is clipped to max_norm (skipped when max_norm <= 0), then AdamW with decoupled weight decay and bias
 * correction (torch.optim.AdamW arithmetic [upstream torch]) updates param / exp_avg / exp_avg_sq in place.  `step` is a
 * device scalar holding the number of steps taken so far; it is incremented by the call.  workspace: device floats,
 * egx_adamw_workspace_floats() of them; workspace[1024] holds the clip coefficient of the last call.  grad is left unscaled.
 * Hyper-parameters are doubles, as torch passes them. */
size_t egx_adamw_workspace_floats(void);
int egx_adamw_clip_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, size_t n_clip,
                        float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay, float* step,
                        float* workspace, void* stream);
/* The same, and the single-block launch in the middle also adds 1 to *cursor (the update's minibatch cursor, egx_update_head). */
int egx_adamw_clip_step_cursor(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, size_t n_clip,
                               float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay, float* step,
                               float* workspace, int32_t* cursor, void* stream);
/* The optimiser step of the policy a train handle belongs to, the handle's weight images included: the two small launches of
 * egx_adamw_clip_step (norm partials, constants - the cursor advance with _cursor) and ONE pass over the weights, in which the
 * blocks that make the images of a weight matrix also run AdamW on it (p, g, m, v read once, the images written from the updated
 * values) and further blocks cover the biases: three launches for the four of egx_adamw_clip_step + egx_policy_train_refresh,
 * the same bits everywhere.  Images of OTHER handles still need their egx_policy_train_refresh.
 * egx_policy_train_bind_flat names the flat parameter buffer (n floats) once, outside graph capture: the fused pass is used for
 * calls with that buffer when every entry of the handle's weight table is a whole matrix inside it and no two overlap, and not
 * with EGX_UPDATE_FUSED_TAIL=0 in the environment when the handle was created; otherwise the calls below enqueue the four
 * launches and egx_policy_train_fused_tail() returns 0.  A table that breaks the rule is reported through egx_last_error() after
 * the bind, which still returns 0; the environment switch, being asked for, leaves no message. */
int egx_policy_train_bind_flat(egx_policy_train* h, const float* param, size_t n);
int egx_policy_train_fused_tail(const egx_policy_train* h);
int egx_adamw_clip_step_train(egx_policy_train* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                              size_t n_clip, float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                              float* step, float* workspace, void* stream);
int egx_adamw_clip_step_train_cursor(egx_policy_train* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                                     size_t n_clip, float max_norm, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, float* step, float* workspace, int32_t* cursor, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGOGEN_HIP_H */
