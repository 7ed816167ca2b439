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
// declarations in lbs.h); this file packs the model at load, lays out the workspace, holds the process-wide switches and launches.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include <atomic>
#include "lbs.h"

// the events egx_profile_next_lbs hands over: the next launch of this thread records them around its fused and fix-up launches
static thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;
extern "C" int egx_profile_next_lbs(void* start_event, void* stop_event) {
  g_prof_start = static_cast<hipEvent_t>(start_event);
  g_prof_stop = static_cast<hipEvent_t>(stop_event);
  return EGX_OK;
}

namespace {
constexpr int NLMK = 51, NEXTRA = 21;
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
// host side: packing + C ABI
// ------------------------------------------------------------------------------------------------
template <typename T>
static int upload(T** dptr, const std::vector<T>& h) {
  EGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(dptr), std::max<size_t>(h.size(), 1) * sizeof(T)));
  if (!h.empty()) EGX_HIP_CHECK(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return EGX_OK;
}

extern "C" int egx_body_model_create(const egx_body_model_host* d, egx_body_model** out) {
  EGX_REQUIRE(d && out, "null argument");
  EGX_REQUIRE(d->num_verts > 0 && d->num_markers >= 0, "bad sizes");
  EGX_REQUIRE(d->v_template_host && d->shapedirs_host && d->posedirs_host && d->J_regressor_host && d->parents_host &&
                  d->lbs_weights_host && d->hand_comps_l_host && d->hand_comps_r_host && d->hand_mean_l_host &&
                  d->hand_mean_r_host && d->extra_vids_host && d->lmk_vids_host && d->lmk_bary_host,
              "null model array");
  const int V = d->num_verts, NVT = egx_ceil_div(V, 32), VP = NVT * 32;
  auto* m = new egx_body_model();
  m->V = V; m->NVT = NVT; m->M = d->num_markers;

  // Joint-coherent vertex order: vertices are sorted by the set of joints they are bound to, so that the 32 vertices
  // of a tile share few joints and the skinning loop of the epilogue (one pass per joint of the tile) stays short
  // (synthetic body: 9.8 -> 4.7 joints per tile).  perm[new] = original vertex id (-1 for the padding rows); every
  // table below is laid out in the new order, outputs are addressed through `vorig` / pick slots.
  std::vector<int> perm(VP, -1);
  {
    std::vector<std::vector<int>> key(V);
    for (int v = 0; v < V; ++v)
      for (int j = 0; j < NJ; ++j)
        if (d->lbs_weights_host[(size_t)v * NJ + j] != 0.f) key[v].push_back(j);
    std::vector<int> order(V);
    for (int v = 0; v < V; ++v) order[v] = v;
    bool natural = false;
#ifdef EGX_LBS_DEVELOPMENT
    if (const char* e = getenv("EGX_LBS_VERTEX_ORDER")) natural = std::string(e) == "natural";
#endif
    // The vertices the environment reads (markers, vertex joints, landmark corners: 241 of 10 475) come FIRST, packed into
    // ceil(241 / 32) = 8 tiles: a call that asks for neither all vertices nor SDF counts (box / crowd / EgoBody scenes, reset
    // tables, get_jts / get_markers) then evaluates 8 vertex tiles instead of every tile that happens to hold one of them
    // (~half of the 328 under the joint order alone).  Both parts keep the joint-coherent order among themselves.
    std::vector<char> is_pick(V, 0);
    auto mark = [&](const int* ids, int n) {
      for (int i = 0; i < n; ++i)
        if (ids[i] >= 0 && ids[i] < V) is_pick[ids[i]] = 1;   // out-of-range ids are reported below (slot_of)
    };
    if (d->marker_vids_host) mark(d->marker_vids_host, d->num_markers);
    mark(d->extra_vids_host, NEXTRA);
    mark(d->lmk_vids_host, NLMK * 3);
    if (!natural)
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        if (is_pick[a] != is_pick[b]) return is_pick[a] > is_pick[b];
        return key[a] < key[b];
      });
    for (int v = 0; v < V; ++v) perm[v] = order[v];
  }

  // blend bases in MFMA A-operand order: [vt][g][c][lane] float4, element e <-> k = 2*(4g+e) + (lane>>5)
  std::vector<f32x4> dirs((size_t)NVT * KGROUPS * 3 * 64);
  for (int vt = 0; vt < NVT; ++vt)
    for (int g = 0; g < KGROUPS; ++g)
      for (int c = 0; c < 3; ++c)
        for (int l = 0; l < 64; ++l) {
          const int v = perm[vt * 32 + (l & 31)];
          f32x4 val = {0.f, 0.f, 0.f, 0.f};
          if (v >= 0)
            for (int e = 0; e < 4; ++e) {
              const int k = 2 * (4 * g + e) + (l >> 5);
              if (k < 10) {
                val[e] = d->shapedirs_host[((size_t)v * 3 + c) * 10 + k];
              } else if (k < KACT) {
                const int jc = (k - 10) / 9, e9 = (k - 10) % 9;
                const int j = jc + 1 + (jc >= 21 ? 3 : 0);        // inverse of egx_compact_joint
                val[e] = d->posedirs_host[(size_t)((j - 1) * 9 + e9) * 3 * V + (size_t)v * 3 + c];
              } else if (k == KACT) {
                val[e] = d->v_template_host[(size_t)v * 3 + c];  // multiplied by the constant-1 feature
              }
            }
          dirs[(((size_t)vt * KGROUPS + g) * 3 + c) * 64 + l] = val;
        }

  // the same bases vertex-major (one vertex's 3 x 472 columns contiguous): the single-vertex fp32 re-evaluation of the mixed blend
  // reads 5.7 KB per vertex from here instead of 720 scattered cache lines of the MFMA-ordered images
  std::vector<float> dirs_rm((size_t)VP * 3 * KDIM, 0.f);
  for (int vn = 0; vn < VP; ++vn) {
    const int v = perm[vn];
    if (v < 0) continue;
    for (int c = 0; c < 3; ++c) {
      float* dst = &dirs_rm[((size_t)vn * 3 + c) * KDIM];
      for (int k = 0; k < 10; ++k) dst[k] = d->shapedirs_host[((size_t)v * 3 + c) * 10 + k];
      for (int k = 10; k < KACT; ++k) {
        const int jc = (k - 10) / 9, e9 = (k - 10) % 9;
        const int j = jc + 1 + (jc >= 21 ? 3 : 0);
        dst[k] = d->posedirs_host[(size_t)((j - 1) * 9 + e9) * 3 * V + (size_t)v * 3 + c];
      }
      dst[KACT] = d->v_template_host[(size_t)v * 3 + c];
    }
  }

  // the same bases as three bf16 planes in the A-operand order of v_mfma_f32_32x32x16_bf16:
  // [vt][s][plane][c][lane] 8 x bf16, element e <-> k = 16 s + 8 (lane>>5) + e, row = lane & 31
  std::vector<unsigned short> dirs3((size_t)NVT * KS3 * 9 * 64 * 8, 0);
  for (int vt = 0; vt < NVT; ++vt)
    for (int sidx = 0; sidx < KS3; ++sidx)
      for (int c = 0; c < 3; ++c)
        for (int l = 0; l < 64; ++l) {
          const int v = perm[vt * 32 + (l & 31)];
          if (v < 0) continue;
          for (int e = 0; e < 8; ++e) {
            const int k = 16 * sidx + 8 * (l >> 5) + e;
            float val = 0.f;
            if (k < 10) {
              val = d->shapedirs_host[((size_t)v * 3 + c) * 10 + k];
            } else if (k < KACT) {
              const int jc = (k - 10) / 9, e9 = (k - 10) % 9;
              const int j = jc + 1 + (jc >= 21 ? 3 : 0);
              val = d->posedirs_host[(size_t)((j - 1) * 9 + e9) * 3 * V + (size_t)v * 3 + c];
            } else if (k == KACT) {
              val = d->v_template_host[(size_t)v * 3 + c];
            } else if (k == KACT + 1) {  // what two bf16 terms of the template leave over (feature 470 selects it)
              const float t = d->v_template_host[(size_t)v * 3 + c];
              unsigned short ht[3];
              egx_bf16_split3(t, ht);
              val = (t - egx_bf16_to_f32(ht[0])) - egx_bf16_to_f32(ht[1]);
            }
            unsigned short h[3];
            egx_bf16_split3(val, h);
            for (int pl = 0; pl < 3; ++pl)
              dirs3[(((((size_t)vt * KS3 + sidx) * 3 + pl) * 3 + c) * 64 + l) * 8 + e] = h[pl];
          }
        }

  // the mixed-blend image (mode 3): the same values, k-steps 0 and 29 as two bf16 planes, k-steps 1..28 as one fp16 plane
  std::vector<unsigned short> dirs4((size_t)NVT * M4_BASE_PIECES * 64 * 8, 0);
  for (int vt = 0; vt < NVT; ++vt)
    for (int sidx = 0; sidx < KS3; ++sidx)
      for (int c = 0; c < 3; ++c)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 8; ++e) {
            const size_t src = (((((size_t)vt * KS3 + sidx) * 3 + 0) * 3 + c) * 64 + l) * 8 + e;      // plane 0 of dirs3
            const size_t pstride = (size_t)3 * 64 * 8;                                               // plane stride in dirs3
            if (sidx == 0 || sidx == KS3 - 1) {
              for (int pl = 0; pl < 2; ++pl)
                dirs4[(((size_t)vt * M4_BASE_PIECES + egx_m4_base_piece(sidx, pl, c)) * 64 + l) * 8 + e] = dirs3[src + pl * pstride];
            } else {
              const float val = egx_bf16_to_f32(dirs3[src]) + egx_bf16_to_f32(dirs3[src + pstride]) + egx_bf16_to_f32(dirs3[src + 2 * pstride]);
              dirs4[(((size_t)vt * M4_BASE_PIECES + egx_m4_base_piece(sidx, 0, c)) * 64 + l) * 8 + e] = egx_f16_rne(val);
            }
          }

  // skinning weights -> per-tile joint lists: the joints any of the tile's 32 vertices is bound to, with the dense
  // [32] weight column of each.  The epilogue walks this list once per body tile (one transform fetch per joint
  // instead of one per vertex and weight).
  int NW = 1;
  for (int v = 0; v < V; ++v) {
    int c = 0;
    for (int j = 0; j < NJ; ++j) c += d->lbs_weights_host[(size_t)v * NJ + j] != 0.f;
    NW = std::max(NW, c);
  }
  m->NW = NW;
  std::vector<int> tj_off(NVT + 1, 0), tj_idx;
  std::vector<float> tj_w;
  for (int vt = 0; vt < NVT; ++vt) {
    for (int j = 0; j < NJ; ++j) {
      float col[32];
      bool any = false;
      for (int r = 0; r < 32; ++r) {
        const int v = perm[vt * 32 + r];
        col[r] = (v >= 0) ? d->lbs_weights_host[(size_t)v * NJ + j] : 0.f;
        any |= col[r] != 0.f;
      }
      if (any) {
        // bits 8..11: which groups of eight rows (rows 8g .. 8g+7 = the four rows of row group g in both lane halves of the
        // epilogue) hold a non-zero weight of this joint - the epilogue skips the others with a scalar test
        int gmask = 0;
        for (int r = 0; r < 32; ++r) gmask |= (col[r] != 0.f) ? (1 << (r >> 3)) : 0;
        tj_idx.push_back(j | (gmask << 8));
        tj_w.insert(tj_w.end(), col, col + 32);
      }
    }
    if ((int)tj_idx.size() == tj_off[vt]) {  // a tile without any weight still needs one (zero) entry
      tj_idx.push_back(0);
      tj_w.insert(tj_w.end(), 32, 0.f);
    }
    tj_off[vt + 1] = (int)tj_idx.size();
  }

  // matrix-pipe skinning weights of every tile (lbs_epilogue_cell): k-step ks covers joints list[8 ks .. 8 ks + 7] of the tile
  std::vector<int> skin_ks_off(NVT + 1, 0);
  for (int vt = 0; vt < NVT; ++vt) skin_ks_off[vt + 1] = skin_ks_off[vt] + (tj_off[vt + 1] - tj_off[vt] + 7) / 8;
  std::vector<unsigned short> skinW((size_t)skin_ks_off[NVT] * 2 * 64 * 8, 0);
  for (int vt = 0; vt < NVT; ++vt) {
    const int JT = tj_off[vt + 1] - tj_off[vt];
    for (int ks = 0; ks < (JT + 7) / 8; ++ks)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
          const int jj = 8 * ks + e;
          if (jj >= JT) continue;
          unsigned short hh[3];
          egx_bf16_split3(tj_w[(size_t)(tj_off[vt] + jj) * 32 + (l & 31)], hh);
          const size_t base = ((size_t)(skin_ks_off[vt] + ks) * 2) * 64 * 8;
          skinW[base + (size_t)l * 8 + e] = hh[0];                                   // operand 0: W_hi in both lane halves
          if (l < 32) skinW[base + (size_t)(64 + l) * 8 + e] = hh[1];                // operand 1: W_mid in lane half 0, zero in half 1
        }
  }

  // picked vertices (markers, vertex joints, landmark corners)
  std::vector<int> pick_slot(VP, -1), marker_slot(d->num_markers), extra_slot(NEXTRA), lmk_slot(NLMK * 3);
  int NP = 0;
  std::vector<int> inv(V);  // original vertex id -> position in the sorted order
  for (int vn = 0; vn < V; ++vn) inv[perm[vn]] = vn;
  auto slot_of = [&](int v) -> int {
    if (v < 0 || v >= V) return -1;
    if (pick_slot[inv[v]] < 0) pick_slot[inv[v]] = NP++;
    return pick_slot[inv[v]];
  };
  bool ok = true;
  for (int i = 0; i < d->num_markers; ++i) ok &= (marker_slot[i] = slot_of(d->marker_vids_host[i])) >= 0;
  for (int i = 0; i < NEXTRA; ++i) ok &= (extra_slot[i] = slot_of(d->extra_vids_host[i])) >= 0;
  for (int i = 0; i < NLMK * 3; ++i) ok &= (lmk_slot[i] = slot_of(d->lmk_vids_host[i])) >= 0;
  if (!ok) { delete m; egx_set_error("vertex id out of range in marker/extra/landmark tables"); return EGX_ERR_ARG; }
  m->NP = NP;
  std::vector<int> pick_tiles;
  for (int vt = 0; vt < NVT; ++vt) {
    bool any = false;
    for (int r = 0; r < 32; ++r) any |= pick_slot[vt * 32 + r] >= 0;
    if (any) pick_tiles.push_back(vt);
  }
  m->n_pick_tiles = (int)pick_tiles.size();
  std::vector<uint8_t> vflags(VP, 0);
  for (int v = 0; v < V; ++v) vflags[v] = 2;
  for (int i = 0; i < d->num_feet; ++i) {
    const int v = d->feet_vids_host[i];
    if (v < 0 || v >= V) { delete m; egx_set_error("feet vertex id out of range"); return EGX_ERR_ARG; }
    vflags[inv[v]] |= 1;
  }
  std::vector<int> sdf_tiles;   // tiles of feet vertices only (and no pick) contribute nothing to a picks + SDF-count call
  for (int vt = 0; vt < NVT; ++vt) {
    bool any = false;
    for (int r = 0; r < 32; ++r) any |= pick_slot[vt * 32 + r] >= 0 || (vflags[vt * 32 + r] & 3) == 2;
    if (any) sdf_tiles.push_back(vt);
  }
  m->n_sdf_tiles = (int)sdf_tiles.size();
  for (int vt : sdf_tiles)
    for (int r = 0; r < 32; ++r) m->verts_sdf_tiles += (vflags[vt * 32 + r] & 2) ? 1 : 0;
  for (int vt : pick_tiles)
    for (int r = 0; r < 32; ++r) m->verts_pick_tiles += (vflags[vt * 32 + r] & 2) ? 1 : 0;
  std::vector<float> lmk_bary(d->lmk_bary_host, d->lmk_bary_host + NLMK * 3);

  // pose constants; joint regression folded through the shape space in double precision:
  //   J(betas) = J_regressor (v_template + shapedirs betas) = J_template + J_shapedirs betas
  std::vector<PoseConsts> pcv(1);
  PoseConsts& pc = pcv[0];
  std::memset(&pc, 0, sizeof(pc));
  pc.max_depth = 0;
  for (int j = 0; j < NJ; ++j) {
    pc.parents[j] = d->parents_host[j];
    if (j > 0 && (pc.parents[j] < 0 || pc.parents[j] >= j)) { delete m; egx_set_error("parents must be topologically ordered"); return EGX_ERR_ARG; }
    pc.depth[j] = (j == 0) ? 0 : pc.depth[pc.parents[j]] + 1;
    pc.max_depth = std::max(pc.max_depth, pc.depth[j]);
  }
  pc.parents[0] = -1;
  for (int j = 0; j < NJ; ++j)
    for (int c = 0; c < 3; ++c) {
      double s = 0.0;
      double sd[10] = {0};
      for (int v = 0; v < V; ++v) {
        const double w = d->J_regressor_host[(size_t)j * V + v];
        if (w == 0.0) continue;
        s += w * d->v_template_host[(size_t)v * 3 + c];
        for (int k = 0; k < 10; ++k) sd[k] += w * d->shapedirs_host[((size_t)v * 3 + c) * 10 + k];
      }
      pc.J_template[j * 3 + c] = (float)s;
      for (int k = 0; k < 10; ++k) pc.J_shapedirs[(j * 3 + c) * 10 + k] = (float)sd[k];
    }
  {   // constants of the fix-up band of the mixed blend (see LBS_FIX_SLACK_M), rounded up to fp32
    auto up = [](double x) { return (float)(x * (1.0 + 1e-6)); };
    std::vector<double> pf(V, 0.0), dpf(V, 0.0);
    for (int j = 1; j < NJ; ++j) {
      const bool movable = j < 22 || j > 24;   // jaw and eyes have no feature: their columns are not in the product
      double mx = 0.0, mxd = 0.0;
      for (int e9 = 0; e9 < 9; ++e9) {
        const int k = movable ? 10 + egx_compact_joint(j) * 9 + e9 : -1;
        const bool fp16_col = k >= 16 && k < 464;
        for (int v = 0; v < V; ++v) {
          double q = 0.0, qd = 0.0;
          for (int c = 0; c < 3; ++c) {
            const float b = d->posedirs_host[(size_t)((j - 1) * 9 + e9) * 3 * V + (size_t)v * 3 + c];
            const double dd = fp16_col ? (double)(float)(_Float16)b - (double)b : 0.0;   // the fp16 plane of dirs4 (egx_f16_rne)
            q += (double)b * b;
            qd += dd * dd;
          }
          mx = std::max(mx, q);
          mxd = std::max(mxd, qd);
          if (movable) { pf[v] += q; dpf[v] += qd; }
        }
      }
      pc.fix_c[j] = up(std::sqrt(mx));
      pc.fix_d[j] = up(std::sqrt(mxd));
    }
    double mpf = 0.0, mdpf = 0.0, mvt = 0.0, mw = 0.0;
    for (int v = 0; v < V; ++v) {
      mpf = std::max(mpf, pf[v]);
      mdpf = std::max(mdpf, dpf[v]);
      double q = 0.0, w = 0.0;
      for (int c = 0; c < 3; ++c) q += (double)d->v_template_host[(size_t)v * 3 + c] * d->v_template_host[(size_t)v * 3 + c];
      for (int j = 0; j < NJ; ++j) w += std::fabs((double)d->lbs_weights_host[(size_t)v * NJ + j]);
      mvt = std::max(mvt, q);
      mw = std::max(mw, w);
    }
    pc.fix_pf = up(std::sqrt(mpf));
    pc.fix_dpf = up(std::sqrt(mdpf));
    pc.vt_max = up(std::sqrt(mvt));
    pc.w_abs_max = up(mw);
    for (int k = 0; k < 10; ++k) {
      double mx = 0.0;
      for (int v = 0; v < V; ++v) {
        double q = 0.0;
        for (int c = 0; c < 3; ++c) q += (double)d->shapedirs_host[((size_t)v * 3 + c) * 10 + k] * d->shapedirs_host[((size_t)v * 3 + c) * 10 + k];
        mx = std::max(mx, q);
      }
      pc.shape_c[k] = up(std::sqrt(mx));
    }
  }
  std::memcpy(pc.hand_comps, d->hand_comps_l_host, 12 * 45 * sizeof(float));
  std::memcpy(pc.hand_comps + 12 * 45, d->hand_comps_r_host, 12 * 45 * sizeof(float));
  std::memcpy(pc.hand_mean, d->hand_mean_l_host, 45 * sizeof(float));
  std::memcpy(pc.hand_mean + 45, d->hand_mean_r_host, 45 * sizeof(float));

  // ---- bounds for the free-space culling of SDF work items.  A posed vertex is a convex combination over its joints j of
  // R_j (v~ - J_j) + p_j (p_j: posed joint, J_j: shaped rest joint, v~: template + shape and pose offsets), so it lies in the
  // convex hull of the balls B(p_j, |v~ - J_j|), and
  //   |v~ - J_j| <= |v_t - J_t,j| + sum_k |beta_k| |S_k,v - JS_k,j| + sum_j' ||R_j' - I||_F ||P_j',v||_F
  // (Cauchy-Schwarz per joint block of the pose blend shapes).  Per tile: D0 = max of the first term over the vertices bound
  // to the joint, E = the maxima of the coefficient norms over the tile's vertices (and its joints, for the shape term).
  std::vector<float> cull_E((size_t)NVT * 64, 0.f), cull_D0(tj_idx.size(), 0.f);
  bool convex = true;
  for (int v = 0; v < V && convex; ++v) {
    double sum = 0.0;
    for (int j = 0; j < NJ; ++j) {
      const float wv = d->lbs_weights_host[(size_t)v * NJ + j];
      if (wv < 0.f) convex = false;
      sum += wv;
    }
    if (std::fabs(sum - 1.0) > 1e-4) convex = false;
  }
  {
    bool lead = pick_tiles.size() <= sdf_tiles.size();
    for (size_t i = 0; i < pick_tiles.size() && lead; ++i) lead = sdf_tiles[i] == pick_tiles[i];
    m->sdf_lead_picks = lead ? 1 : 0;
  }
  // the culled launch treats the first n_pick_tiles entries of the SDF tile list as "always evaluated"
  for (size_t i = 0; i < pick_tiles.size() && convex; ++i) convex = i < sdf_tiles.size() && sdf_tiles[i] == pick_tiles[i];
  m->cull_ok = convex ? 1 : 0;
  for (int c = 0; c < 3; ++c) m->rest_pelvis[c] = pc.J_template[c];
  for (int vt = 0; vt < NVT && convex; ++vt) {
    float* E = &cull_E[(size_t)vt * 64];
    for (int r = 0; r < 32; ++r) {
      const int v = perm[vt * 32 + r];
      if (v < 0) continue;
      for (int jj = tj_off[vt]; jj < tj_off[vt + 1]; ++jj) {
        const int j = tj_idx[jj] & 0xff;
        if (d->lbs_weights_host[(size_t)v * NJ + j] != 0.f) {
          double q = 0.0;
          for (int c = 0; c < 3; ++c) {
            const double e = (double)d->v_template_host[(size_t)v * 3 + c] - (double)pc.J_template[j * 3 + c];
            q += e * e;
          }
          cull_D0[jj] = std::max(cull_D0[jj], (float)(std::sqrt(q) * (1.0 + 1e-6)));
        }
        for (int k = 0; k < 10; ++k) {   // shape term, over every joint of the tile's list (a superset of the vertex's own)
          double q = 0.0;
          for (int c = 0; c < 3; ++c) {
            const double e = (double)d->shapedirs_host[((size_t)v * 3 + c) * 10 + k] - (double)pc.J_shapedirs[(j * 3 + c) * 10 + k];
            q += e * e;
          }
          E[k] = std::max(E[k], (float)(std::sqrt(q) * (1.0 + 1e-6)));
        }
      }
      for (int jc = 0; jc < 51; ++jc) {
        const int j = jc + 1 + (jc >= 21 ? 3 : 0);
        double q = 0.0;
        for (int e9 = 0; e9 < 9; ++e9)
          for (int c = 0; c < 3; ++c) {
            const double e = d->posedirs_host[(size_t)((j - 1) * 9 + e9) * 3 * V + (size_t)v * 3 + c];
            q += e * e;
          }
        E[10 + jc] = std::max(E[10 + jc], (float)(std::sqrt(q) * (1.0 + 1e-6)));
      }
    }
  }

  // The bound is only worth evaluating where it is tight: at a reference pose (|beta_k| = 0.8, ||R_j - I||_F = 0.42, i.e.
  // 0.3 rad at every joint) the blend-shape margin of the median tile must stay below 15 cm.  Learned body models pass (shape
  // directions are smooth fields, pose correctives act near their joint: centimetres); a model whose blend shapes are
  // i.i.d. noise in all 469 x 3V entries - the synthetic benchmark body of SURVEY 8(d) - does not (0.56 m: no box is ever
  // free), and its launches skip the three culling kernels altogether.
  if (convex) {
    std::vector<float> ref(NVT);
    for (int vt = 0; vt < NVT; ++vt) {
      float mg = 0.f;
      for (int i = 0; i < 10; ++i) mg += 0.8f * cull_E[(size_t)vt * 64 + i];
      for (int i = 10; i < 61; ++i) mg += 0.42f * cull_E[(size_t)vt * 64 + i];
      ref[vt] = mg;
    }
    std::nth_element(ref.begin(), ref.begin() + NVT / 2, ref.end());
    m->cull_ref_margin = ref[NVT / 2];
    if (m->cull_ref_margin > 0.15f) m->cull_ok = 0;
  }

  int rc = EGX_OK;
  if ((rc = upload(&m->cull_E, cull_E)) || (rc = upload(&m->cull_D0, cull_D0))) { egx_body_model_destroy(m); return rc; }
  {
    unsigned short* d3 = nullptr;
    if ((rc = upload(&d3, dirs3))) { egx_body_model_destroy(m); return rc; }
    m->dirs3 = reinterpret_cast<bf16x8*>(d3);
    unsigned short* d4 = nullptr;
    if ((rc = upload(&d4, dirs4))) { egx_body_model_destroy(m); return rc; }
    m->dirs4 = reinterpret_cast<bf16x8*>(d4);
  }
  {
    unsigned short* sw = nullptr;
    if ((rc = upload(&sw, skinW)) || (rc = upload(&m->skin_ks_off, skin_ks_off)) || (rc = upload(&m->dirs_rm, dirs_rm))) { egx_body_model_destroy(m); return rc; }
    m->skinW = reinterpret_cast<bf16x8*>(sw);
  }
  if ((rc = upload(&m->vorig, perm)) || (rc = upload(&m->pick_tiles, pick_tiles)) ||
      (rc = upload(&m->sdf_tiles, sdf_tiles))) { egx_body_model_destroy(m); return rc; }
  if ((rc = upload(&m->dirs, dirs)) || (rc = upload(&m->tj_off, tj_off)) || (rc = upload(&m->tj_idx, tj_idx)) ||
      (rc = upload(&m->tj_w, tj_w)) || (rc = upload(&m->pick_slot, pick_slot)) || (rc = upload(&m->vflags, vflags)) ||
      (rc = upload(&m->pc, pcv)) || (rc = upload(&m->marker_slot, marker_slot)) || (rc = upload(&m->extra_slot, extra_slot)) ||
      (rc = upload(&m->lmk_slot, lmk_slot)) || (rc = upload(&m->lmk_bary, lmk_bary))) {
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
// blend mode of the fused kernel: 0 = fp32 MFMA, 1 = 3-term bf16 split, 2 = 2-term bf16 split, 3 = mixed (2-term bf16 shape / template +
// fp16 pose correctives, the default); vertex-writing calls always use 0
std::atomic<int> g_blend_mode{-1};
int blend_mode() {
  int m = g_blend_mode.load();
  if (m < 0) {
    const char* e = getenv("EGX_LBS_BLEND");
    const std::string v = e ? e : "";
    // unset = f16mix (mode 3: counts re-evaluated in fp32 where the cheap product cannot decide); an unknown string is an
    // error of the call that reads it (-2), not a silent default
    m = (v == "f32" || v == "0") ? 0 : ((v == "bf16x3" || v == "1") ? 1 : ((v == "bf16x2" || v == "2") ? 2 : ((v.empty() || v == "f16mix" || v == "3") ? 3 : -2)));
    if (m >= 0) g_blend_mode.store(m);
  }
  return m;
}
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
// free-space culling of SDF work items: OPT-IN (EGX_LBS_CULL=1 / egx_lbs_set_culling(1)).  Measured on MI355X, 10 240 bodies,
// structured body (profiles/r04_lbs_culling.md): freshly reset agents standing in the room - 60 % of the items evaluated, fused
// kernel 1.13 -> 0.77 ms, the three culling kernels + 0.11 ms; bodies inside geometry or outside the room (what a random-init
// policy produces, i.e. the benchmark loop): nothing to skip, + 0.11 ms.  A win for trained policies on learned body models, a
// loss in the benchmark loop, hence not the default.
std::atomic<int> g_cull{-1};
int culling_on() {
  int c = g_cull.load();
  if (c < 0) {
    const char* e = getenv("EGX_LBS_CULL");
    c = (e && std::string(e) == "1") ? 1 : 0;
    g_cull.store(c);
  }
  return c;
}
}  // namespace

namespace {
// wave tile of the mixed-blend kernel: 0 = by launch size (see egx_lbs_forward), 1 = 32 x 32 (three workgroups per CU), 2 = 32 x 64
std::atomic<int> g_wave_tile{-1};
int wave_tile() {
  int t = g_wave_tile.load();
  if (t < 0) {
    const char* e = getenv("EGX_LBS_WAVE_TILE");
    t = e ? atoi(e) : 0;
    g_wave_tile.store(t);
  }
  return t;
}
}  // namespace

namespace {
std::atomic<int> g_fixq_cap{0};   // 0 = LBS_FIXQ_CAP
}
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
  lbs_launch_pose(false, static_cast<hipStream_t>(stream_), m->pc, xb, betas, B, fpa, nullptr, nullptr, reinterpret_cast<f32x4*>(ws + wl.A4),
                  out_joints55, NJ, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                  SdfDev{}, nullptr, nullptr, 0);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

// ------------------------------------------------------------------------------------------------
// SDF scene sets: the per-scene records of egx_lbs_forward_scenes, made once (struct egx_sdf_scene_set: egx_common.h)
// ------------------------------------------------------------------------------------------------

extern "C" int egx_sdf_scene_set_create(const egx_sdf_grid* scenes, int num_scenes, egx_sdf_scene_set** out) {
  EGX_REQUIRE(scenes && out, "null argument");
  EGX_REQUIRE(num_scenes >= 1 && num_scenes < (1 << 15), "a scene set holds 1 .. 32767 scenes");   // the fused kernels queue the index in 15 bits
  std::vector<SdfSceneDev> rec((size_t)num_scenes);
  const egx_sdf_grid& s0 = scenes[0];
  // every check comes before the first device access (the slope reads below): a rejected set touches no pointer it was given
  for (int i = 0; i < num_scenes; ++i) {
    const egx_sdf_grid& g = scenes[i];
    if (g.d0 != s0.d0 || g.d1 != s0.d1 || g.d2 != s0.d2) {
      egx_set_error("egx_sdf_scene_set_create: scene " + std::to_string(i) + " has grid dimensions " + std::to_string(g.d0) + "x" +
                    std::to_string(g.d1) + "x" + std::to_string(g.d2) + ", scene 0 " + std::to_string(s0.d0) + "x" +
                    std::to_string(s0.d1) + "x" + std::to_string(s0.d2) + ": the scenes of a set share their dimensions");
      return EGX_ERR_ARG;
    }
  }
  for (int i = 0; i < num_scenes; ++i) {
    const egx_sdf_grid& g = scenes[i];
    if (!g.grid || !g.coarse_minmax || !egx_sdf_dims_ok(g.d0, g.d1, g.d2) || g.d0 <= 0 || g.d1 <= 0) {
      egx_set_error("egx_sdf_scene_set_create: scene " + std::to_string(i) +
                    " needs a grid with d2 >= 2 and fewer than 2^32 samples and its bracket table (egx_sdf_build_coarse)");
      return EGX_ERR_ARG;
    }
  }
  // the slopes (aux[3] of each table) were written by egx_sdf_build_coarse on some stream: wait for it, then read them once
  EGX_HIP_CHECK(hipDeviceSynchronize());
  const int c0 = egx_ceil_div(s0.d0, 4), c1 = egx_ceil_div(s0.d1, 4), c2 = egx_ceil_div(s0.d2, 4);
  for (int i = 0; i < num_scenes; ++i) {
    const egx_sdf_grid& g = scenes[i];
    SdfSceneDev& r = rec[(size_t)i];
    r.grid = g.grid;
    r.coarse = static_cast<const float2*>(g.coarse_minmax);
    r.cx = g.center[0]; r.cy = g.center[1]; r.cz = g.center[2]; r.scale = g.scale;
    EGX_HIP_CHECK(hipMemcpy(&r.slope, static_cast<const char*>(g.coarse_minmax) + egx_sdf_aux_offset(c0, c1, c2) + 3 * sizeof(float),
                            sizeof(float), hipMemcpyDeviceToHost));
    r.pad = 0.f;
  }
  auto* set = new egx_sdf_scene_set();
  set->S = num_scenes;
  set->dims = s0;
  if (int rc = upload(&set->table, rec)) { (void)hipFree(set->table); delete set; return rc; }
  *out = set;
  return EGX_OK;
}

extern "C" void egx_sdf_scene_set_destroy(egx_sdf_scene_set* set) {
  if (!set) return;
  (void)hipFree(set->table);
  delete set;
}

extern "C" int egx_sdf_scene_set_size(const egx_sdf_scene_set* set) { return set ? set->S : 0; }

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
  EGX_REQUIRE(!sdf || (sdf->grid && out_pene_count && sdf->d0 > 0 && sdf->d1 > 0 && sdf->d2 > 0), "sdf needs grid + out_pene_count");
  EGX_REQUIRE(!sdf || sdf->coarse_minmax, "sdf needs its bracket table: call egx_sdf_build_coarse once per grid");
  EGX_REQUIRE(!sdf || egx_sdf_dims_ok(sdf->d0, sdf->d1, sdf->d2), "sdf grid needs d2 >= 2 and fewer than 2^32 samples");
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
  SdfDev sd;
  std::memset(&sd, 0, sizeof(sd));
  const float* mips = nullptr;
  if (sdf) {
    sd.grid = sdf->grid; sd.d0 = sdf->d0; sd.d1 = sdf->d1; sd.d2 = sdf->d2;
    sd.cx = sdf->center[0]; sd.cy = sdf->center[1]; sd.cz = sdf->center[2]; sd.scale = sdf->scale;
    sd.coarse = static_cast<const float2*>(sdf->coarse_minmax);
    sd.c0 = egx_ceil_div(sdf->d0, 4); sd.c1 = egx_ceil_div(sdf->d1, 4); sd.c2 = egx_ceil_div(sdf->d2, 4);
    mips = reinterpret_cast<const float*>(static_cast<const char*>(sdf->coarse_minmax) + egx_sdf_table_bytes(sd.c0, sd.c1, sd.c2));
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
  lbs_launch_pose(ms, stream, m->pc, xb, betas, B, fpa,
                  split3 ? nullptr : feat, split3 ? reinterpret_cast<unsigned short*>(feat) : nullptr, A4, out_joints,
                  EGX_NUM_JOINTS_OUT, (split3 && mode >= 2) ? 1.f : 0.f, (split3 && mode == 3) ? feat4 : nullptr, sdf ? out_pene_count : nullptr,
                  static_cast<const int*>(order), fvec, jpos, (int)wl.Bp, fix ? reinterpret_cast<float*>(ws + wl.fix_e) : nullptr,
                  reinterpret_cast<int*>(ws + wl.fix_stats), fix ? reinterpret_cast<unsigned short*>(ws + wl.skinB) : nullptr,
                  reinterpret_cast<f32x4*>(ws + wl.cinit), R0, T0, sd, scene_tab, static_cast<const int*>(agent_scene), n_scenes);
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
    p.sdf_aux = (sdf && !ms) ? reinterpret_cast<const float*>(static_cast<const char*>(sdf->coarse_minmax) + egx_sdf_aux_offset(sd.c0, sd.c1, sd.c2)) : nullptr;
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
