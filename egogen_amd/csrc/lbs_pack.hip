// Packing of a body description at load: vertex order, the four images of the blend bases, the per-tile joint lists and skinning
// weights, the pick slots and tile lists, the pose constants, the constants of the fix-up band and the culling bounds.  Host code
// only, no HIP runtime call (see lbs_pack.h); lbs_pack_model at the end of the file is the sequence of the steps.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "lbs_pack.h"

bool lbs_joint_depths(const int32_t* parents, int* depth, int* max_depth) {
  depth[0] = 0;
  *max_depth = 0;
  for (int j = 1; j < NJ; ++j) {
    if (parents[j] < 0 || parents[j] >= j) return false;
    depth[j] = depth[parents[j]] + 1;
    *max_depth = std::max(*max_depth, depth[j]);
  }
  return true;
}

void lbs_fold_joint_regressor(const egx_body_model_host* d, float* Jt, float* Jsd) {
  const int V = d->num_verts;
  for (int j = 0; j < NJ; ++j) {
    double t[3] = {0, 0, 0}, s[30] = {0};
    for (int v = 0; v < V; ++v) {
      const double r = d->J_regressor_host[(size_t)j * V + v];
      if (r == 0.0) continue;
      for (int c = 0; c < 3; ++c) t[c] += r * d->v_template_host[(size_t)v * 3 + c];
      for (int e = 0; e < 30; ++e) s[e] += r * d->shapedirs_host[(size_t)v * 30 + e];
    }
    for (int c = 0; c < 3; ++c) Jt[3 * j + c] = (float)t[c];
    for (int e = 0; e < 30; ++e) Jsd[(size_t)j * 30 + e] = (float)s[e];
  }
}

namespace {

// The blend bases of a description.  col(v, c, k) is column k of the blend GEMM for coordinate c of vertex v:
//   k < 10 shapedirs | k < KACT posedirs of joint egx_expand_joint((k - 10) / 9), entry (k - 10) % 9 | k == KACT the template
//   (multiplied by the constant-1 feature) | 0 in the padding columns
struct Bases {
  const egx_body_model_host* d;
  float shape(int v, int c, int k) const { return d->shapedirs_host[((size_t)v * 3 + c) * 10 + k]; }
  float pose(int j, int e9, int v, int c) const {   // j in 1..54: jaw and eyes included, which have no column
    return d->posedirs_host[(size_t)((j - 1) * 9 + e9) * 3 * d->num_verts + (size_t)v * 3 + c];
  }
  float tmpl(int v, int c) const { return d->v_template_host[(size_t)v * 3 + c]; }
  float col(int v, int c, int k) const {
    if (k < 10) return shape(v, c, k);
    if (k < KACT) return pose(egx_expand_joint((k - 10) / 9), (k - 10) % 9, v, c);
    return k == KACT ? tmpl(v, c) : 0.f;
  }
  float weight(int v, int j) const { return d->lbs_weights_host[(size_t)v * NJ + j]; }
};

float up(double x) { return (float)(x * (1.0 + 1e-6)); }   // a float64 bound, rounded up to fp32

// The same column of sorted row vn (0 in the padding rows), read back from the vertex-major image once pack_dirs_rm has made it:
// contiguous per vertex, where the description's pose directions are 3V floats apart from column to column.
inline float packed_col(const LbsPacked& p, int vn, int c, int k) { return k < KDIM ? p.dirs_rm[((size_t)vn * 3 + c) * KDIM + k] : 0.f; }

// Joint-coherent vertex order: vertices are sorted by the set of joints they are bound to, so that the 32 vertices
// of a tile share few joints and the skinning loop of the epilogue (one pass per joint of the tile) stays short
// (synthetic body: 9.8 -> 4.7 joints per tile).  perm[new] = original vertex id (-1 for the padding rows); every
// table below is laid out in the new order, outputs are addressed through `vorig` / pick slots.
void pack_vertex_order(const Bases& b, LbsPacked& p) {
  const egx_body_model_host* d = b.d;
  const int V = p.V;
  p.perm.assign((size_t)p.NVT * 32, -1);
  std::vector<std::vector<int>> key(V);
  for (int v = 0; v < V; ++v)
    for (int j = 0; j < NJ; ++j)
      if (b.weight(v, j) != 0.f) key[v].push_back(j);
  for (int v = 0; v < V; ++v) p.perm[v] = v;
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
      if (ids[i] >= 0 && ids[i] < V) is_pick[ids[i]] = 1;   // out-of-range ids are reported by pack_picks
  };
  if (d->marker_vids_host) mark(d->marker_vids_host, d->num_markers);
  mark(d->extra_vids_host, NEXTRA);
  mark(d->lmk_vids_host, NLMK * 3);
  if (!natural)
    std::stable_sort(p.perm.begin(), p.perm.begin() + V, [&](int a, int b) {
      if (is_pick[a] != is_pick[b]) return is_pick[a] > is_pick[b];
      return key[a] < key[b];
    });
}

// the blend bases vertex-major (one vertex's 3 x 472 columns contiguous): the single-vertex fp32 re-evaluation of the mixed blend
// reads 5.7 KB per vertex from here instead of 720 scattered cache lines of the MFMA-ordered images
void pack_dirs_rm(const Bases& b, LbsPacked& p) {
  p.dirs_rm.assign((size_t)p.NVT * 32 * 3 * KDIM, 0.f);
  for (int vn = 0; vn < p.NVT * 32; ++vn) {
    const int v = p.perm[vn];
    if (v < 0) continue;
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k <= KACT; ++k) p.dirs_rm[((size_t)vn * 3 + c) * KDIM + k] = b.col(v, c, k);
  }
}

// the same bases in MFMA A-operand order: [vt][g][c][lane] float4, element e <-> k = 2*(4g+e) + (lane>>5)
void pack_dirs(LbsPacked& p) {
  p.dirs.resize((size_t)p.NVT * KGROUPS * 3 * 64);
  for (int vt = 0; vt < p.NVT; ++vt)
    for (int g = 0; g < KGROUPS; ++g)
      for (int c = 0; c < 3; ++c)
        for (int l = 0; l < 64; ++l) {
          f32x4 val;
          for (int e = 0; e < 4; ++e) val[e] = packed_col(p, vt * 32 + (l & 31), c, 2 * (4 * g + e) + (l >> 5));
          p.dirs[(((size_t)vt * KGROUPS + g) * 3 + c) * 64 + l] = val;
        }
}

// the same bases as three bf16 planes in the A-operand order of v_mfma_f32_32x32x16_bf16:
// [vt][s][plane][c][lane] 8 x bf16, element e <-> k = 16 s + 8 (lane>>5) + e, row = lane & 31
void pack_dirs3(LbsPacked& p) {
  p.dirs3.assign((size_t)p.NVT * KS3 * 9 * 64 * 8, 0);
  for (int vt = 0; vt < p.NVT; ++vt)
    for (int sidx = 0; sidx < KS3; ++sidx)
      for (int c = 0; c < 3; ++c)
        for (int l = 0; l < 64; ++l) {
          const int vn = vt * 32 + (l & 31);
          if (p.perm[vn] < 0) continue;
          for (int e = 0; e < 8; ++e) {
            const int k = 16 * sidx + 8 * (l >> 5) + e;
            float val = packed_col(p, vn, c, k);
            if (k == KACT + 1) {  // what two bf16 terms of the template leave over (feature 470 selects it)
              const float t = packed_col(p, vn, c, KACT);
              unsigned short ht[3];
              egx_bf16_split3(t, ht);
              val = (t - egx_bf16_to_f32(ht[0])) - egx_bf16_to_f32(ht[1]);
            }
            unsigned short h[3];
            egx_bf16_split3(val, h);
            for (int pl = 0; pl < 3; ++pl)
              p.dirs3[(((((size_t)vt * KS3 + sidx) * 3 + pl) * 3 + c) * 64 + l) * 8 + e] = h[pl];
          }
        }
}

// the mixed-blend image (mode 3): the values of dirs3, k-steps 0 and 29 as two bf16 planes, k-steps 1..28 as one fp16 plane
void pack_dirs4(LbsPacked& p) {
  const std::vector<unsigned short>& dirs3 = p.dirs3;
  p.dirs4.assign((size_t)p.NVT * M4_BASE_PIECES * 64 * 8, 0);
  for (int vt = 0; vt < p.NVT; ++vt)
    for (int sidx = 0; sidx < KS3; ++sidx)
      for (int c = 0; c < 3; ++c)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 8; ++e) {
            const size_t src = (((((size_t)vt * KS3 + sidx) * 3 + 0) * 3 + c) * 64 + l) * 8 + e;      // plane 0 of dirs3
            const size_t pstride = (size_t)3 * 64 * 8;                                               // plane stride in dirs3
            if (sidx == 0 || sidx == KS3 - 1) {
              for (int pl = 0; pl < 2; ++pl)
                p.dirs4[(((size_t)vt * M4_BASE_PIECES + egx_m4_base_piece(sidx, pl, c)) * 64 + l) * 8 + e] = dirs3[src + pl * pstride];
            } else {
              const float val = egx_bf16_to_f32(dirs3[src]) + egx_bf16_to_f32(dirs3[src + pstride]) + egx_bf16_to_f32(dirs3[src + 2 * pstride]);
              p.dirs4[(((size_t)vt * M4_BASE_PIECES + egx_m4_base_piece(sidx, 0, c)) * 64 + l) * 8 + e] = egx_f16_rne(val);
            }
          }
}

// skinning weights -> per-tile joint lists: the joints any of the tile's 32 vertices is bound to, with the dense
// [32] weight column of each.  The epilogue walks this list once per body tile (one transform fetch per joint
// instead of one per vertex and weight).
void pack_tile_joints(const Bases& b, LbsPacked& p) {
  p.NW = 1;
  for (int v = 0; v < p.V; ++v) {
    int c = 0;
    for (int j = 0; j < NJ; ++j) c += b.weight(v, j) != 0.f;
    p.NW = std::max(p.NW, c);
  }
  p.tj_off.assign(p.NVT + 1, 0);
  for (int vt = 0; vt < p.NVT; ++vt) {
    for (int j = 0; j < NJ; ++j) {
      float col[32];
      bool any = false;
      for (int r = 0; r < 32; ++r) {
        const int v = p.perm[vt * 32 + r];
        col[r] = (v >= 0) ? b.weight(v, j) : 0.f;
        any |= col[r] != 0.f;
      }
      if (any) {
        // bits 8..11: which groups of eight rows (rows 8g .. 8g+7 = the four rows of row group g in both lane halves of the
        // epilogue) hold a non-zero weight of this joint - the epilogue skips the others with a scalar test
        int gmask = 0;
        for (int r = 0; r < 32; ++r) gmask |= (col[r] != 0.f) ? (1 << (r >> 3)) : 0;
        p.tj_idx.push_back(j | (gmask << 8));
        p.tj_w.insert(p.tj_w.end(), col, col + 32);
      }
    }
    if ((int)p.tj_idx.size() == p.tj_off[vt]) {  // a tile without any weight still needs one (zero) entry
      p.tj_idx.push_back(0);
      p.tj_w.insert(p.tj_w.end(), 32, 0.f);
    }
    p.tj_off[vt + 1] = (int)p.tj_idx.size();
  }
}

// matrix-pipe skinning weights of every tile (lbs_epilogue_cell): k-step ks covers joints list[8 ks .. 8 ks + 7] of the tile
void pack_skin_weights(LbsPacked& p) {
  p.skin_ks_off.assign(p.NVT + 1, 0);
  for (int vt = 0; vt < p.NVT; ++vt) p.skin_ks_off[vt + 1] = p.skin_ks_off[vt] + (p.tj_off[vt + 1] - p.tj_off[vt] + 7) / 8;
  p.skinW.assign((size_t)p.skin_ks_off[p.NVT] * 2 * 64 * 8, 0);
  for (int vt = 0; vt < p.NVT; ++vt) {
    const int JT = p.tj_off[vt + 1] - p.tj_off[vt];
    for (int ks = 0; ks < (JT + 7) / 8; ++ks)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
          const int jj = 8 * ks + e;
          if (jj >= JT) continue;
          unsigned short hh[3];
          egx_bf16_split3(p.tj_w[(size_t)(p.tj_off[vt] + jj) * 32 + (l & 31)], hh);
          const size_t base = ((size_t)(p.skin_ks_off[vt] + ks) * 2) * 64 * 8;
          p.skinW[base + (size_t)l * 8 + e] = hh[0];                                   // operand 0: W_hi in both lane halves
          if (l < 32) p.skinW[base + (size_t)(64 + l) * 8 + e] = hh[1];                // operand 1: W_mid in lane half 0, zero in half 1
        }
  }
}

// picked vertices (markers, vertex joints, landmark corners): one slot per distinct vertex; the feet flags; and the two tile lists,
// the tiles a markers-and-joints call evaluates and the ones a call with SDF counts does
int pack_picks(const egx_body_model_host* d, LbsPacked& p) {
  const int V = p.V, VP = p.NVT * 32;
  p.pick_slot.assign(VP, -1);
  p.marker_slot.resize(d->num_markers);
  p.extra_slot.resize(NEXTRA);
  p.lmk_slot.resize(NLMK * 3);
  std::vector<int> inv(V);  // original vertex id -> position in the sorted order
  for (int vn = 0; vn < V; ++vn) inv[p.perm[vn]] = vn;
  auto slot_of = [&](int v) -> int {
    if (v < 0 || v >= V) return -1;
    if (p.pick_slot[inv[v]] < 0) p.pick_slot[inv[v]] = p.NP++;
    return p.pick_slot[inv[v]];
  };
  bool ok = true;
  for (int i = 0; i < d->num_markers; ++i) ok &= (p.marker_slot[i] = slot_of(d->marker_vids_host[i])) >= 0;
  for (int i = 0; i < NEXTRA; ++i) ok &= (p.extra_slot[i] = slot_of(d->extra_vids_host[i])) >= 0;
  for (int i = 0; i < NLMK * 3; ++i) ok &= (p.lmk_slot[i] = slot_of(d->lmk_vids_host[i])) >= 0;
  if (!ok) { egx_set_error("vertex id out of range in marker/extra/landmark tables"); return EGX_ERR_ARG; }
  p.lmk_bary.assign(d->lmk_bary_host, d->lmk_bary_host + NLMK * 3);
  p.vflags.assign(VP, 0);
  for (int v = 0; v < V; ++v) p.vflags[v] = 2;
  for (int i = 0; i < d->num_feet; ++i) {
    const int v = d->feet_vids_host[i];
    if (v < 0 || v >= V) { egx_set_error("feet vertex id out of range"); return EGX_ERR_ARG; }
    p.vflags[inv[v]] |= 1;
  }
  for (int vt = 0; vt < p.NVT; ++vt) {
    bool pick = false, count = false;   // tiles of feet vertices only (and no pick) contribute nothing to a picks + SDF-count call
    for (int r = 0; r < 32; ++r) {
      pick |= p.pick_slot[vt * 32 + r] >= 0;
      count |= (p.vflags[vt * 32 + r] & 3) == 2;
    }
    if (pick) p.pick_tiles.push_back(vt);
    if (pick || count) p.sdf_tiles.push_back(vt);
  }
  p.n_pick_tiles = (int)p.pick_tiles.size();
  p.n_sdf_tiles = (int)p.sdf_tiles.size();
  for (int vt : p.sdf_tiles)
    for (int r = 0; r < 32; ++r) p.verts_sdf_tiles += (p.vflags[vt * 32 + r] & 2) ? 1 : 0;
  for (int vt : p.pick_tiles)
    for (int r = 0; r < 32; ++r) p.verts_pick_tiles += (p.vflags[vt * 32 + r] & 2) ? 1 : 0;
  // mode 3 treats the leading n_pick_tiles entries of the SDF tile list as the precise ones
  bool lead = p.pick_tiles.size() <= p.sdf_tiles.size();
  for (size_t i = 0; i < p.pick_tiles.size() && lead; ++i) lead = p.sdf_tiles[i] == p.pick_tiles[i];
  p.sdf_lead_picks = lead ? 1 : 0;
  return EGX_OK;
}

// the kinematic tree, the folded joint regressor and the hand PCA tables
int pack_pose_consts(const egx_body_model_host* d, PoseConsts& pc) {
  std::memset(&pc, 0, sizeof(pc));
  for (int j = 0; j < NJ; ++j) pc.parents[j] = d->parents_host[j];
  if (!lbs_joint_depths(d->parents_host, pc.depth, &pc.max_depth)) { egx_set_error("parents must be topologically ordered"); return EGX_ERR_ARG; }
  pc.parents[0] = -1;
  lbs_fold_joint_regressor(d, pc.J_template, pc.J_shapedirs);
  std::memcpy(pc.hand_comps, d->hand_comps_l_host, 12 * 45 * sizeof(float));
  std::memcpy(pc.hand_comps + 12 * 45, d->hand_comps_r_host, 12 * 45 * sizeof(float));
  std::memcpy(pc.hand_mean, d->hand_mean_l_host, 45 * sizeof(float));
  std::memcpy(pc.hand_mean + 45, d->hand_mean_r_host, 45 * sizeof(float));
  return EGX_OK;
}

// constants of the fix-up band of the mixed blend (see LBS_FIX_SLACK_M), rounded up to fp32
void pack_band_consts(const Bases& b, int V, PoseConsts& pc) {
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
          const float x = b.pose(j, e9, v, c);
          const double dd = fp16_col ? (double)(float)(_Float16)x - (double)x : 0.0;   // the fp16 plane of dirs4 (egx_f16_rne)
          q += (double)x * x;
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
    for (int c = 0; c < 3; ++c) q += (double)b.tmpl(v, c) * b.tmpl(v, c);
    for (int j = 0; j < NJ; ++j) w += std::fabs((double)b.weight(v, j));
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
      for (int c = 0; c < 3; ++c) q += (double)b.shape(v, c, k) * b.shape(v, c, k);
      mx = std::max(mx, q);
    }
    pc.shape_c[k] = up(std::sqrt(mx));
  }
}

// Bounds for the free-space culling of SDF work items.  A posed vertex is a convex combination over its joints j of
// R_j (v~ - J_j) + p_j (p_j: posed joint, J_j: shaped rest joint, v~: template + shape and pose offsets), so it lies in the
// convex hull of the balls B(p_j, |v~ - J_j|), and
//   |v~ - J_j| <= |v_t - J_t,j| + sum_k |beta_k| |S_k,v - JS_k,j| + sum_j' ||R_j' - I||_F ||P_j',v||_F
// (Cauchy-Schwarz per joint block of the pose blend shapes).  Per tile: D0 = max of the first term over the vertices bound
// to the joint, E = the maxima of the coefficient norms over the tile's vertices (and its joints, for the shape term).
void pack_cull_bounds(const Bases& b, LbsPacked& p) {
  const PoseConsts& pc = p.pc[0];
  p.cull_E.assign((size_t)p.NVT * 64, 0.f);
  p.cull_D0.assign(p.tj_idx.size(), 0.f);
  bool convex = true;
  for (int v = 0; v < p.V && convex; ++v) {
    double sum = 0.0;
    for (int j = 0; j < NJ; ++j) {
      const float wv = b.weight(v, j);
      if (wv < 0.f) convex = false;
      sum += wv;
    }
    if (std::fabs(sum - 1.0) > 1e-4) convex = false;
  }
  // the culled launch treats the first n_pick_tiles entries of the SDF tile list as "always evaluated"
  convex = convex && p.sdf_lead_picks;
  p.cull_ok = convex ? 1 : 0;
  for (int c = 0; c < 3; ++c) p.rest_pelvis[c] = pc.J_template[c];
  for (int vt = 0; vt < p.NVT && convex; ++vt) {
    float* E = &p.cull_E[(size_t)vt * 64];
    for (int r = 0; r < 32; ++r) {
      const int v = p.perm[vt * 32 + r];
      if (v < 0) continue;
      for (int jj = p.tj_off[vt]; jj < p.tj_off[vt + 1]; ++jj) {
        const int j = p.tj_idx[jj] & 0xff;
        if (b.weight(v, j) != 0.f) {
          double q = 0.0;
          for (int c = 0; c < 3; ++c) {
            const double e = (double)b.tmpl(v, c) - (double)pc.J_template[j * 3 + c];
            q += e * e;
          }
          p.cull_D0[jj] = std::max(p.cull_D0[jj], up(std::sqrt(q)));
        }
        for (int k = 0; k < 10; ++k) {   // shape term, over every joint of the tile's list (a superset of the vertex's own)
          double q = 0.0;
          for (int c = 0; c < 3; ++c) {
            const double e = (double)packed_col(p, vt * 32 + r, c, k) - (double)pc.J_shapedirs[(j * 3 + c) * 10 + k];
            q += e * e;
          }
          E[k] = std::max(E[k], up(std::sqrt(q)));
        }
      }
      for (int jc = 0; jc < 51; ++jc) {
        double q = 0.0;
        for (int e9 = 0; e9 < 9; ++e9)
          for (int c = 0; c < 3; ++c) {
            const double e = packed_col(p, vt * 32 + r, c, 10 + jc * 9 + e9);
            q += e * e;
          }
        E[10 + jc] = std::max(E[10 + jc], up(std::sqrt(q)));
      }
    }
  }
  if (!convex) return;
  // The bound is only worth evaluating where it is tight: at a reference pose (|beta_k| = 0.8, ||R_j - I||_F = 0.42, i.e.
  // 0.3 rad at every joint) the blend-shape margin of the median tile must stay below 15 cm.  Learned body models pass (shape
  // directions are smooth fields, pose correctives act near their joint: centimetres); a model whose blend shapes are
  // i.i.d. noise in all 469 x 3V entries - the synthetic benchmark body of SURVEY 8(d) - does not (0.56 m: no box is ever
  // free), and its launches skip the three culling kernels altogether.
  std::vector<float> ref(p.NVT);
  for (int vt = 0; vt < p.NVT; ++vt) {
    float mg = 0.f;
    for (int i = 0; i < 10; ++i) mg += 0.8f * p.cull_E[(size_t)vt * 64 + i];
    for (int i = 10; i < 61; ++i) mg += 0.42f * p.cull_E[(size_t)vt * 64 + i];
    ref[vt] = mg;
  }
  std::nth_element(ref.begin(), ref.begin() + p.NVT / 2, ref.end());
  p.cull_ref_margin = ref[p.NVT / 2];
  if (p.cull_ref_margin > 0.15f) p.cull_ok = 0;
}

}  // namespace

int lbs_pack_model(const egx_body_model_host* d, LbsPacked* out) {
  EGX_REQUIRE(d && out, "null argument");
  EGX_REQUIRE(d->num_verts > 0 && d->num_markers >= 0, "bad sizes");
  EGX_REQUIRE(d->v_template_host && d->shapedirs_host && d->posedirs_host && d->J_regressor_host && d->parents_host &&
                  d->lbs_weights_host && d->hand_comps_l_host && d->hand_comps_r_host && d->hand_mean_l_host &&
                  d->hand_mean_r_host && d->extra_vids_host && d->lmk_vids_host && d->lmk_bary_host,
              "null model array");
  LbsPacked& p = *out;
  p = LbsPacked();
  p.V = d->num_verts; p.NVT = egx_ceil_div(p.V, 32); p.M = d->num_markers;
  p.pc.resize(1);
  const Bases b{d};
  pack_vertex_order(b, p);
  pack_dirs_rm(b, p);
  pack_dirs(p);
  pack_dirs3(p);
  pack_dirs4(p);
  pack_tile_joints(b, p);
  pack_skin_weights(p);
  int rc = pack_picks(d, p);
  if (!rc) rc = pack_pose_consts(d, p.pc[0]);
  if (rc) { p = LbsPacked(); return rc; }   // an error leaves nothing packed
  pack_band_consts(b, p.V, p.pc[0]);
  pack_cull_bounds(b, p);
  return EGX_OK;
}
