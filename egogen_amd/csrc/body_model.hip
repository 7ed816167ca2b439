// SMPL-X forward for gfx950: pose/chain kernel + fused blend-shape GEMM (fp32 MFMA) / skinning /
// SDF-count / vertex-pick kernel + joints/markers gather kernel, behind the C ABI of include/egogen_hip.h.
//
// What the reference does (models/baseops.py:338-398 -> smplx.SMPLX.forward [upstream]):
//   v_posed = v_template + [betas | vec(R_1..54 - I)] @ [shapedirs ; posedirs]      (B x 496 x 3V GEMM)
//   A       = rigid chain over 55 joints (relative to the rest joints)
//   verts   = (sum_j W[v,j] A_j) [v_posed;1] + transl
// and then only ever consumes markers, joints and (crowd_env_2f.py:163-175) the per-frame count of
// vertices whose scene SDF is negative.  Layout decisions for MI355X:
//   * the blend GEMM runs on v_mfma_f32_32x32x2_f32 with rows = vertices, cols = bodies and three
//     accumulator sets (x,y,z) so each lane ends up owning complete (vertex, body) points;
//   * both operands are pre-packed in exactly the lane order of the MFMA operands, 4 k-steps per
//     16-byte load, so every global load is a fully coalesced 1 KiB wave access;
//   * skinning weights are ELL-packed (nnz per vertex found at load time), joint transforms are
//     written body-minor ([tile][joint][row][32 bodies] float4) so the epilogue reads are coalesced;
//   * the vertex tensor never has to exist: SDF counting and the ~240 picked vertices are epilogues.
// The kernels live in one file per family (lbs_pose.hip, lbs_fused.hip, lbs_fused3.hip, lbs_fix.hip, lbs_cull.hip; shared
// declarations in lbs.h) and the model is packed at load by lbs_pack.hip, host code a CPU test checks byte by byte; this file holds
// the gather kernel, uploads the packed model, lays out the workspace, holds the process-wide switches and launches.
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "egx_sdf.h"
#include "lbs_pack.h"

// the events egx_profile_next_lbs hands over: the next launch of this thread records them around its fused and fix-up launches
static thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;
extern "C" int egx_profile_next_lbs(void* start_event, void* stop_event) {
  g_prof_start = static_cast<hipEvent_t>(start_event);
  g_prof_stop = static_cast<hipEvent_t>(stop_event);
  return EGX_OK;
}

namespace {
constexpr int BODY_PAD = 256;          // bodies per workgroup of the fused kernel
}  // namespace

// ------------------------------------------------------------------------------------------------
// kernel 3: assemble joints[55..126] and markers from the picked vertices
// ------------------------------------------------------------------------------------------------
__global__ void egx_gather_kernel(const float* __restrict__ picked, int B, int NP, int M,
                                  const int* __restrict__ marker_slot, const int* __restrict__ extra_slot,
                                  const int* __restrict__ lmk_slot, const float* __restrict__ lmk_bary,
                                  float* __restrict__ out_joints, float* __restrict__ out_markers) {
  const int b = blockIdx.x;
  const float* pk = picked + (size_t)b * NP * 3;
  for (int i = threadIdx.x; i < M + NEXTRA + NLMK; i += blockDim.x) {
    if (i < M) {
      if (out_markers) {
        const float* s = pk + marker_slot[i] * 3;
        float* o = out_markers + ((size_t)b * M + i) * 3;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
      }
    } else if (out_joints) {
      float* o = out_joints + ((size_t)b * EGX_NUM_JOINTS_OUT + NJ + (i - M)) * 3;
      if (i < M + NEXTRA) {
        const float* s = pk + extra_slot[i - M] * 3;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
      } else {
        const int l = i - M - NEXTRA;
        float acc[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; ++k) {
          const float* s = pk + lmk_slot[l * 3 + k] * 3;
          const float w = lmk_bary[l * 3 + k];
          acc[0] += s[0] * w; acc[1] += s[1] * w; acc[2] += s[2] * w;
        }
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side: the loaded model (packed by lbs_pack.hip, uploaded here) + C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int egx_body_model_create(const egx_body_model_host* d, egx_body_model** out) {
  EGX_REQUIRE(d && out, "null argument");
  LbsPacked p;
  if (int rc = lbs_pack_model(d, &p)) return rc;
  auto* m = new egx_body_model();
  static_cast<LbsModelDims&>(*m) = p;
  auto u16 = [](bf16x8** dptr) { return reinterpret_cast<unsigned short**>(dptr); };   // the 16-bit images are packed as plain shorts
  int rc = EGX_OK;
  if ((rc = egx_upload(&m->cull_E, p.cull_E)) || (rc = egx_upload(&m->cull_D0, p.cull_D0)) || (rc = egx_upload(u16(&m->dirs3), p.dirs3)) ||
      (rc = egx_upload(u16(&m->dirs4), p.dirs4)) || (rc = egx_upload(u16(&m->skinW), p.skinW)) || (rc = egx_upload(&m->skin_ks_off, p.skin_ks_off)) ||
      (rc = egx_upload(&m->dirs_rm, p.dirs_rm)) || (rc = egx_upload(&m->vorig, p.perm)) || (rc = egx_upload(&m->pick_tiles, p.pick_tiles)) ||
      (rc = egx_upload(&m->sdf_tiles, p.sdf_tiles)) || (rc = egx_upload(&m->dirs, p.dirs)) || (rc = egx_upload(&m->tj_off, p.tj_off)) ||
      (rc = egx_upload(&m->tj_idx, p.tj_idx)) || (rc = egx_upload(&m->tj_w, p.tj_w)) || (rc = egx_upload(&m->pick_slot, p.pick_slot)) ||
      (rc = egx_upload(&m->vflags, p.vflags)) || (rc = egx_upload(&m->pc, p.pc)) || (rc = egx_upload(&m->marker_slot, p.marker_slot)) ||
      (rc = egx_upload(&m->extra_slot, p.extra_slot)) || (rc = egx_upload(&m->lmk_slot, p.lmk_slot)) ||
      (rc = egx_upload(&m->lmk_bary, p.lmk_bary))) {
    egx_body_model_destroy(m);
    return rc;
  }
  *out = m;
  return EGX_OK;
}

extern "C" void egx_body_model_destroy(egx_body_model* m) {
  if (!m) return;
  (void)hipFree(m->dirs); (void)hipFree(m->dirs3); (void)hipFree(m->dirs4); (void)hipFree(m->tj_off); (void)hipFree(m->tj_idx); (void)hipFree(m->tj_w);
  (void)hipFree(m->pick_slot); (void)hipFree(m->pick_tiles); (void)hipFree(m->sdf_tiles); (void)hipFree(m->vflags); (void)hipFree(m->vorig); (void)hipFree(m->pc); (void)hipFree(m->marker_slot);
  (void)hipFree(m->extra_slot); (void)hipFree(m->lmk_slot); (void)hipFree(m->lmk_bary);
  (void)hipFree(m->cull_E); (void)hipFree(m->cull_D0);
  (void)hipFree(m->skinW); (void)hipFree(m->skin_ks_off); (void)hipFree(m->dirs_rm);
  delete m;
}

extern "C" int egx_body_model_num_verts(const egx_body_model* m) { return m ? m->V : 0; }
extern "C" int egx_body_model_nnz(const egx_body_model* m) { return m ? m->NW : 0; }
extern "C" int egx_body_model_lbs_vertices(const egx_body_model* m, int with_sdf) {
  return m ? (with_sdf ? m->verts_sdf_tiles : m->verts_pick_tiles) : 0;
}

namespace {
// ---- process-wide switches: set through the C ABI, else read from the environment once (the first call that asks)
template <typename Parse>
int switch_value(std::atomic<int>& g, const char* env_name, Parse&& parse) {
  int v = g.load();
  if (v < 0) {
    const char* e = getenv(env_name);
    v = parse(std::string(e ? e : ""));
    if (v >= 0) g.store(v);
  }
  return v;
}
// blend mode of the fused kernel: 0 = fp32 MFMA, 1 = 3-term bf16 split, 2 = 2-term bf16 split, 3 = mixed (2-term bf16 shape / template +
// fp16 pose correctives, the default); vertex-writing calls always use 0
std::atomic<int> g_blend_mode{-1};
int blend_mode() {
  // unset = f16mix (mode 3: counts re-evaluated in fp32 where the cheap product cannot decide); an unknown string is an
  // error of the call that reads it (-2), not a silent default
  return switch_value(g_blend_mode, "EGX_LBS_BLEND", [](const std::string& v) {
    return (v == "f32" || v == "0") ? 0 : ((v == "bf16x3" || v == "1") ? 1 : ((v == "bf16x2" || v == "2") ? 2 : ((v.empty() || v == "f16mix" || v == "3") ? 3 : -2)));
  });
}
// free-space culling of SDF work items: OPT-IN (EGX_LBS_CULL=1 / egx_lbs_set_culling(1)).  Measured on MI355X, 10 240 bodies,
// structured body (profiles/r04_lbs_culling.md): freshly reset agents standing in the room - 60 % of the items evaluated, fused
// kernel 1.13 -> 0.77 ms, the three culling kernels + 0.11 ms; bodies inside geometry or outside the room (what a random-init
// policy produces, i.e. the benchmark loop): nothing to skip, + 0.11 ms.  A win for trained policies on learned body models, a
// loss in the benchmark loop, hence not the default.
std::atomic<int> g_cull{-1};
int culling_on() {
  return switch_value(g_cull, "EGX_LBS_CULL", [](const std::string& v) { return v == "1" ? 1 : 0; });
}
// wave tile of the mixed-blend kernel: 0 = by launch size (see egx_lbs_forward), 1 = 32 x 32 (three workgroups per CU), 2 = 32 x 64
std::atomic<int> g_wave_tile{-1};
int wave_tile() {
  return switch_value(g_wave_tile, "EGX_LBS_WAVE_TILE", [](const std::string& v) { return atoi(v.c_str()); });
}
std::atomic<int> g_fixq_cap{0};   // fix-up queue entries per sub-queue in use, 0 = LBS_FIXQ_CAP

struct WsLayout {
  size_t feat, feat4, A4, picked, total;
  // culled SDF launches
  size_t fvec, jpos, order, flags, items, counts;
  size_t fix_e, fix_stats;   // fix-up of the mixed blend: per-slot error bound, counter of re-evaluated vertices
  size_t skinB, cinit;       // matrix-pipe skinning operands of the mixed blend
  size_t fixq;               // fix-up queue
  size_t Bp;
  int items_stride;
};
WsLayout ws_layout(const egx_body_model* m, int B) {
  const size_t Bp = egx_align_up((size_t)B, BODY_PAD);
  WsLayout w;
  w.Bp = Bp;
  w.feat = 0;
  w.feat4 = egx_align_up(w.feat + Bp * std::max<size_t>(KDIM * sizeof(float), (size_t)KS3 * 16 * 3 * 2), 256);   // mixed-blend features (mode 3)
  w.A4 = egx_align_up(w.feat4 + Bp * ((size_t)M4_FEAT_PIECES * 64 * 16 / 32), 256);   // 32 KiB per 32-body tile
  w.picked = egx_align_up(w.A4 + Bp * NJ * 12 * sizeof(float), 256);
  w.fvec = egx_align_up(w.picked + (size_t)B * m->NP * 3 * sizeof(float), 256);
  w.jpos = egx_align_up(w.fvec + 64 * Bp * sizeof(float), 256);
  w.order = egx_align_up(w.jpos + (size_t)NJ * 3 * Bp * sizeof(float), 256);
  w.flags = egx_align_up(w.order + (size_t)B * sizeof(int), 256);
  const size_t n_items = (size_t)m->n_sdf_tiles * (Bp / BODY_PAD);
  w.items_stride = (int)n_items;
  w.items = egx_align_up(w.flags + n_items * sizeof(int), 256);
  w.counts = egx_align_up(w.items + 8 * n_items * sizeof(int), 256);
  w.fix_e = egx_align_up(w.counts + 16 * sizeof(int), 256);
  w.fix_stats = egx_align_up(w.fix_e + Bp * sizeof(float), 256);
  w.skinB = egx_align_up(w.fix_stats + LBS_FIX_STATS_INTS * sizeof(int), 256);
  w.cinit = egx_align_up(w.skinB + (Bp / 32) * (size_t)SKIN_BT_BYTES, 256);
  w.fixq = egx_align_up(w.cinit + Bp * sizeof(f32x4), 256);
  w.total = egx_align_up(w.fixq + (size_t)LBS_FIX_NQ * LBS_FIXQ_CAP * sizeof(int2), 256);
  return w;
}
}  // namespace

extern "C" int egx_lbs_set_fix_queue_capacity(int entries) {
  EGX_REQUIRE(entries >= 0 && entries <= LBS_FIXQ_CAP, "capacity must be 0 (default) .. the workspace's queue size");
  g_fixq_cap.store(entries);
  return EGX_OK;
}

extern "C" int egx_lbs_set_wave_tile(int tile) {
  EGX_REQUIRE(tile >= 0 && tile <= 2, "wave tile must be 0 (by launch size), 1 (32 x 32) or 2 (32 x 64)");
  g_wave_tile.store(tile);
  return EGX_OK;
}
extern "C" int egx_lbs_get_wave_tile(void) { return wave_tile(); }

extern "C" int egx_lbs_set_culling(int on) {
  g_cull.store(on ? 1 : 0);
  return EGX_OK;
}
extern "C" int egx_lbs_get_culling(void) { return culling_on(); }
extern "C" int egx_body_model_culls(const egx_body_model* m, float* out_reference_margin_m) {
  if (!m) return 0;
  if (out_reference_margin_m) *out_reference_margin_m = m->cull_ref_margin;
  return m->cull_ok;
}

extern "C" int egx_lbs_cull_stats(const egx_body_model* m, const void* workspace, int num_bodies, int32_t* out_active_items,
                                  int32_t* out_total_items) {
  EGX_REQUIRE(m && workspace && num_bodies > 0 && out_active_items && out_total_items, "bad arguments");
  const WsLayout wl = ws_layout(m, num_bodies);
  int c[16];
  EGX_HIP_CHECK(hipMemcpy(c, static_cast<const char*>(workspace) + wl.counts, sizeof(c), hipMemcpyDeviceToHost));
  if (c[15] != 0x43554c4c) {
    egx_set_error("egx_lbs_cull_stats: no culled launch has run on this workspace (culling off, a model whose bound is not tight, "
                  "a call without SDF counts, or the fp32 blend mode)");
    return EGX_ERR_ARG;
  }
  *out_active_items = c[8];
  *out_total_items = wl.items_stride;
  return EGX_OK;
}

extern "C" int egx_lbs_fix_stats(const egx_body_model* m, const void* workspace, int num_bodies, int32_t* out_reevaluated) {
  EGX_REQUIRE(m && workspace && num_bodies > 0 && out_reevaluated, "bad arguments");
  const WsLayout wl = ws_layout(m, num_bodies);
  std::vector<int32_t> st(LBS_FIX_STATS_INTS);
  EGX_HIP_CHECK(hipMemcpy(st.data(), static_cast<const char*>(workspace) + wl.fix_stats, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  const int cap = g_fixq_cap.load() > 0 ? g_fixq_cap.load() : LBS_FIXQ_CAP;   // the capacity in force now (= at the launch, unless changed since)
  int64_t n = st[0];                                                            // re-evaluated inside the fused kernel (full sub-queue)
  for (int q = 0; q < LBS_FIX_NQ; ++q) n += std::min(st[LBS_FIX_CNT0 + 32 * q], cap);
  // (entries a wave reserved and then marked void are counted twice: only when a sub-queue overflowed)
  *out_reevaluated = (int32_t)std::min<int64_t>(n, INT32_MAX);
  return EGX_OK;
}

extern "C" int egx_lbs_set_blend_mode(int mode) {
  EGX_REQUIRE(mode >= 0 && mode <= 3, "blend mode must be 0 (fp32 MFMA), 1 (bf16x3 split), 2 (bf16x2 split) or 3 (bf16x2 shape / template + fp16 pose correctives)");
  g_blend_mode.store(mode);
  return EGX_OK;
}
extern "C" int egx_lbs_get_blend_mode(void) { return blend_mode(); }   // < 0: EGX_LBS_BLEND holds an unknown string

extern "C" size_t egx_lbs_workspace_bytes(const egx_body_model* m, int num_bodies) {
  if (!m || num_bodies <= 0) return 0;
  return ws_layout(m, num_bodies).total;
}

extern "C" int egx_lbs_joints(const egx_body_model* m, const float* xb, const float* betas, int B, int fpa, float* out_joints55,
                              void* workspace, size_t workspace_bytes, void* stream_) {
  EGX_REQUIRE(m && xb && betas && out_joints55, "null model/xb/betas/out");
  EGX_REQUIRE(B > 0 && fpa > 0, "num_bodies and frames_per_agent must be positive");
  const WsLayout wl = ws_layout(m, B);
  if (!workspace || workspace_bytes < wl.total) {
    egx_set_error("workspace too small: need " + std::to_string(wl.total) + " bytes");
    return EGX_ERR_WORKSPACE;
  }
  char* ws = static_cast<char*>(workspace);
  LbsPoseArgs a;
  a.pc = m->pc; a.xb = xb; a.betas = betas; a.B = B; a.fpa = fpa;
  a.A4 = reinterpret_cast<f32x4*>(ws + wl.A4);
  a.out_joints = out_joints55; a.joints_ld = NJ;
  lbs_launch_pose(false, static_cast<hipStream_t>(stream_), a);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

// Set of one through the one-scene kernels: bodies whose agent names no scene of the set get the count -1 (after the count was formed).
__global__ __launch_bounds__(256) void egx_lbs_scene_mark_kernel(const int* __restrict__ agent_scene, int n_scenes, int B, int fpa,
                                                                 int* __restrict__ pene) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int v = agent_scene[b / fpa];
  if (v < 0 || v >= n_scenes) pene[b] = -1;
}

// The launcher of egx_lbs_forward (one scene: `sdf`, set = null) and egx_lbs_forward_scenes (`set` with agent_scene; sdf = the set's
// shared dimensions).  Set launches take the MS instantiations of the pose, fused and fix-up kernels and are never culled.
static int lbs_forward_launch(const egx_body_model* m, const float* xb, const float* betas, int B, int fpa,
                              float* out_verts, float* out_joints, float* out_markers, const egx_sdf_grid* sdf,
                              const egx_sdf_scene_set* set, const int32_t* agent_scene,
                              const float* R0, const float* T0, int32_t* out_pene_count, void* workspace,
                              size_t workspace_bytes, void* stream_) {
  EGX_REQUIRE(m && xb && betas, "null model/xb/betas");
  EGX_REQUIRE(B > 0 && fpa > 0, "num_bodies and frames_per_agent must be positive");
  EGX_REQUIRE(!sdf || out_pene_count, "sdf needs out_pene_count");
  EGX_REQUIRE(!sdf || egx_sdf_grid_ok(sdf), "sdf grid needs d2 >= 2 and fewer than 2^32 samples");
  EGX_REQUIRE(!sdf || sdf->coarse_minmax, "sdf needs its bracket table: call egx_sdf_build_coarse once per grid");
  const WsLayout wl = ws_layout(m, B);
  if (!workspace || workspace_bytes < wl.total) {
    egx_set_error("workspace too small: need " + std::to_string(wl.total) + " bytes");
    return EGX_ERR_WORKSPACE;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  float* feat = reinterpret_cast<float*>(ws + wl.feat);
  unsigned short* feat4 = reinterpret_cast<unsigned short*>(ws + wl.feat4);
  f32x4* A4 = reinterpret_cast<f32x4*>(ws + wl.A4);
  const bool need_picks = out_joints || out_markers;
  float* picked = need_picks ? reinterpret_cast<float*>(ws + wl.picked) : nullptr;

  const int mode = blend_mode();   // read ONCE per call: the feature flag of column 470 and the kernel choice must agree
  EGX_REQUIRE(mode >= 0, "EGX_LBS_BLEND must be one of f32 | bf16x3 | bf16x2 | f16mix");
  const bool split3 = mode >= 1 && !out_verts;
  const int nbg_all = egx_ceil_div(B, BODY_PAD);
  // free-space culling: SDF counts on the split kernels, a convex-weight model, whole agents, enough items to deal to 8 XCDs
  const bool ms = set != nullptr;
  const bool cull = !ms && split3 && sdf && m->cull_ok && culling_on() && B % fpa == 0 && m->n_sdf_tiles > m->n_pick_tiles &&
                    (size_t)m->n_sdf_tiles * nbg_all >= 8;
  SdfDev sd = {};
  const float* mips = nullptr;
  const float* aux = nullptr;
  if (sdf) {
    const EgxSdfTables t(*sdf);
    sd = egx_sdf_dev(*sdf);
    sd.coarse = t.brackets();
    mips = t.mips();
    aux = t.aux();
  }
  const bool fix = split3 && mode == 3 && sdf;   // mixed blend with counts: the pose kernel also writes the per-body error bound
  int* order = cull ? reinterpret_cast<int*>(ws + wl.order) : nullptr;
  int* flags = reinterpret_cast<int*>(ws + wl.flags);
  int* items = reinterpret_cast<int*>(ws + wl.items);
  int* counts = reinterpret_cast<int*>(ws + wl.counts);
  float* fvec = cull ? reinterpret_cast<float*>(ws + wl.fvec) : nullptr;
  float* jpos = cull ? reinterpret_cast<float*>(ws + wl.jpos) : nullptr;
  if (cull) lbs_launch_cull_order(m, xb, R0, T0, sd, mips, B, fpa, nbg_all, order, flags, counts, stream);
  const SdfSceneDev* scene_tab = ms ? set->table : nullptr;
  const int n_scenes = ms ? set->S : 0;
  LbsPoseArgs a;
  a.pc = m->pc; a.xb = xb; a.betas = betas; a.B = B; a.fpa = fpa; a.A4 = A4; a.out_joints = out_joints; a.joints_ld = EGX_NUM_JOINTS_OUT;
  if (split3) a.feat3 = reinterpret_cast<unsigned short*>(feat); else a.feat = feat;   // one buffer: bf16 planes or the fp32 operand
  a.template_lo_feat = (split3 && mode >= 2) ? 1.f : 0.f;
  a.feat4 = (split3 && mode == 3) ? feat4 : nullptr;
  a.zero_counts = sdf ? out_pene_count : nullptr;
  a.agent_of_slot = order; a.fvec = fvec; a.jpos = jpos; a.Bp = (int)wl.Bp;
  a.fix_e = fix ? reinterpret_cast<float*>(ws + wl.fix_e) : nullptr;
  a.skinB = fix ? reinterpret_cast<unsigned short*>(ws + wl.skinB) : nullptr;
  a.fix_stats = reinterpret_cast<int*>(ws + wl.fix_stats); a.cinit = reinterpret_cast<f32x4*>(ws + wl.cinit);
  a.R0 = R0; a.T0 = T0; a.sdf = sd; a.scenes = scene_tab; a.agent_scene = agent_scene; a.n_scenes = n_scenes;
  lbs_launch_pose(ms, stream, a);
  if (cull)
    lbs_launch_cull_items(m, fvec, jpos, (int)wl.Bp, order, B, fpa, nbg_all, R0, T0, sd, mips, flags, items, wl.items_stride, counts, stream);
  if (out_verts || need_picks || sdf) {
    LbsParams p;
    p.dirs = m->dirs; p.tj_off = m->tj_off; p.tj_idx = m->tj_idx; p.tj_w = m->tj_w; p.pick_slot = m->pick_slot;
    p.dirs3 = m->dirs3; p.feat3 = reinterpret_cast<const bf16x8*>(feat);
    p.dirs4 = m->dirs4; p.feat4 = reinterpret_cast<const bf16x8*>(feat4);
    p.vorig = m->vorig;
    p.vflags = m->vflags; p.feat = reinterpret_cast<const f32x4*>(feat); p.A4 = A4; p.xb = xb;
    p.B = B; p.V = m->V; p.NVT = m->NVT; p.NW = m->NW; p.NP = m->NP; p.fpa = fpa;
    p.nbg = egx_ceil_div(B, BODY_PAD);
#ifdef EGX_LBS_DEVELOPMENT   // ablation switches of development builds only (make CXXFLAGS+=-DEGX_LBS_DEVELOPMENT)
    {
      const char* e = getenv("EGX_LBS_DBG");
      p.dbg = e ? atoi(e) : 0;
    }
#else
    p.dbg = 0;
#endif
    p.verts = out_verts; p.picked = picked; p.R0 = R0; p.T0 = T0; p.pene = out_pene_count;
    p.agent_of_slot = order; p.items = cull ? items : nullptr; p.item_counts = counts; p.items_stride = wl.items_stride;
    // markers and joints only: the vertex tiles without a picked vertex are never looked at
    // (with SDF counts: nor the tiles made of feet vertices only, which the count excludes)
    p.tiles = out_verts ? nullptr : (sdf ? m->sdf_tiles : m->pick_tiles);
    p.n_tiles = out_verts ? m->NVT : (sdf ? m->n_sdf_tiles : m->n_pick_tiles);
    // mode 3: the tile lists start with the tiles that hold picked vertices (checked at load: sdf_lead_picks)
    p.n_precise = sdf ? (m->sdf_lead_picks ? m->n_pick_tiles : m->n_sdf_tiles) : m->n_pick_tiles;
#ifdef EGX_LBS_DEVELOPMENT
    if (const char* e = getenv("EGX_LBS_PRECISE")) p.n_precise = atoi(e);
#endif
    p.sdf = sd;   // out_pene_count was cleared by the pose kernel above
    p.fix_e = reinterpret_cast<const float*>(ws + wl.fix_e);
    p.fix_stats = reinterpret_cast<int*>(ws + wl.fix_stats);
    p.skinW = m->skinW; p.skin_ks_off = m->skin_ks_off;
    p.fixq = reinterpret_cast<int2*>(ws + wl.fixq); p.fixq_cap = g_fixq_cap.load() > 0 ? g_fixq_cap.load() : LBS_FIXQ_CAP;
    p.dirs_rm = m->dirs_rm; p.pc = m->pc; p.betas = betas;
    p.skinB = reinterpret_cast<const bf16x8*>(ws + wl.skinB); p.cinit = reinterpret_cast<const f32x4*>(ws + wl.cinit);
    p.sdf_aux = ms ? nullptr : aux;
    p.scenes = scene_tab; p.agent_scene = agent_scene; p.n_scenes = n_scenes;
    // three body groups per block: features + joint transforms of a block (3 x 1.2 MB) still live in the XCD's 4 MiB L2 and the
    // bases stream through twice per XCD instead of three times (5 groups per XCD at 10 240 bodies): fabric-side traffic 1.77 ->
    // 1.43 GB per launch at the same launch time (1: 2.6 GB, 5: 1.65 GB and +4 % time; profiles/r04_lbs_traffic.md)
    p.bg_block = 3;
#ifdef EGX_LBS_DEVELOPMENT
    if (const char* e = getenv("EGX_LBS_BG_BLOCK")) p.bg_block = atoi(e);
#endif
    hipEvent_t ev0 = g_prof_start, ev1 = g_prof_stop;
    g_prof_start = g_prof_stop = nullptr;
    if (ev0) EGX_HIP_CHECK(hipEventRecord(ev0, stream));
    // the split blends run the 4-wave kernels of lbs_fused3.hip, blend mode 0 and every vertex-writing call the fp32 kernel of lbs_fused.hip
    if (int rc = split3 ? lbs_launch_fused3(p, mode, sdf != nullptr, ms, wave_tile(), stream) : lbs_launch_fused(p, sdf != nullptr, ms, stream))
      return rc;
    // mixed blend with counts: the vertices the fused kernel queued for the fp32 re-evaluation (inside the profiled interval: it is
    // part of what the mode costs)
    if (fix) lbs_launch_fix(p, ms, stream);
    if (ev1) EGX_HIP_CHECK(hipEventRecord(ev1, stream));
  }
  if (need_picks)
    hipLaunchKernelGGL(egx_gather_kernel, dim3(B), dim3(256), 0, stream, picked, B, m->NP, m->M, m->marker_slot,
                       m->extra_slot, m->lmk_slot, m->lmk_bary, out_joints, out_markers);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_lbs_forward(const egx_body_model* m, const float* xb, const float* betas, int B, int fpa,
                               float* out_verts, float* out_joints, float* out_markers, const egx_sdf_grid* sdf,
                               const float* R0, const float* T0, int32_t* out_pene_count, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return lbs_forward_launch(m, xb, betas, B, fpa, out_verts, out_joints, out_markers, sdf, nullptr, nullptr, R0, T0, out_pene_count,
                            workspace, workspace_bytes, stream);
}

extern "C" int egx_lbs_forward_scenes(const egx_body_model* m, const float* xb, const float* betas, int B, int fpa,
                                      float* out_verts, float* out_joints, float* out_markers, const egx_sdf_scene_set* scenes,
                                      const int32_t* agent_scene, const float* R0, const float* T0, int32_t* out_pene_count,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  EGX_REQUIRE(scenes && agent_scene && out_pene_count, "a scene-set call needs the set, agent_scene and out_pene_count");
  if (scenes->S == 1) {
    // a set of one runs the one-scene kernels (the general ones cost +11 % at 10 240 bodies, profiles/scene_set.md) and may be culled
    // like a one-scene call; the bodies of agents whose index is not 0 then get their -1 behind the launch
    if (int rc = lbs_forward_launch(m, xb, betas, B, fpa, out_verts, out_joints, out_markers, &scenes->dims, nullptr, nullptr, R0, T0,
                                    out_pene_count, workspace, workspace_bytes, stream))
      return rc;
    hipLaunchKernelGGL(egx_lbs_scene_mark_kernel, dim3(egx_ceil_div(B, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), agent_scene,
                       1, B, fpa, out_pene_count);
    EGX_HIP_CHECK(hipGetLastError());
    return EGX_OK;
  }
  return lbs_forward_launch(m, xb, betas, B, fpa, out_verts, out_joints, out_markers, &scenes->dims, scenes, agent_scene, R0, T0,
                            out_pene_count, workspace, workspace_bytes, stream);
}
