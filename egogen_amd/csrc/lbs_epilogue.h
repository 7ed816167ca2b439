// Device code of the fused LBS kernels that more than one kernel file uses: per-wave LDS state and tile metadata, the fp32
// re-evaluation of single vertices (fix-up of the mixed blend) and the VALU epilogue (skinning, SDF count, picks, vertex write).
#pragma once
#include "lbs.h"

// per-wave LDS of the fp32 fused kernel (lbs_fused.hip): metadata of the current vertex tile, then the queue / the transpose buffer
constexpr int LBS_META_BYTES = 7680;                 // s_W[55*32] f32, s_jl[56], s_slot[32], masks[4], s_cnt[64] (16-byte multiple)
constexpr int LBS_VERT_BYTES = 32 * 97 * 4;          // per-wave transpose buffer of the vertex-writing variants
constexpr int LBS_QCAP = 640;                        // entries of the per-wave queue of undecided SDF points (>= 512 + 64)
constexpr int LBS_THREADS = 512;

template <bool WRITE_VERTS, bool DO_SDF>
__device__ __forceinline__ LbsWave lbs_wave_init(char* my, int lane) {
  LbsWave w;
  w.lane = lane; w.n = lane & 31; w.half = lane >> 5;
  w.s_W = reinterpret_cast<float*>(my);
  w.s_jl = reinterpret_cast<int*>(my + NJ * 32 * 4);
  w.s_slot = w.s_jl + 56;
  w.s_masks = reinterpret_cast<unsigned*>(w.s_slot + 32);
  w.s_cnt = reinterpret_cast<int*>(w.s_masks + 4);
  w.lds = reinterpret_cast<float*>(my + LBS_META_BYTES);
  w.s_queue = reinterpret_cast<f32x4*>(my + LBS_META_BYTES);
  w.s_fixmap = nullptr; w.s_thr = nullptr;
  w.qn = 0;
  w.s_cnt[lane] = 0;
  return w;
}

// per-tile metadata, private to the wave (DS operations of one wave execute in order: no barrier)
__device__ __forceinline__ int lbs_load_meta(const LbsParams& p, LbsWave& w, int vt) {
  const int lane = w.lane;
  float* s_W = w.s_W; int* s_jl = w.s_jl; int* s_slot = w.s_slot; unsigned* s_masks = w.s_masks;
  const int j_lo = p.tj_off[vt];
  const int JT = p.tj_off[vt + 1] - j_lo;
  for (int idx = lane * 4; idx < JT * 32; idx += 256)
    *reinterpret_cast<f32x4*>(&s_W[idx]) = *reinterpret_cast<const f32x4*>(&p.tj_w[(size_t)j_lo * 32 + idx]);
  if (lane < JT) s_jl[lane] = p.tj_idx[j_lo + lane];
  {
    const int sl = (lane < 32) ? p.pick_slot[vt * 32 + lane] : -1;
    const int fl = (lane < 32) ? p.vflags[vt * 32 + lane] : 0;
    if (lane < 32) s_slot[lane] = sl;
    const unsigned long long mp = __ballot(sl >= 0), ms = __ballot((fl & 3) == 2);
    if (lane == 0) { s_masks[0] = (unsigned)mp; s_masks[1] = (unsigned)ms; }
  }
  __builtin_amdgcn_wave_barrier();

  return JT;
}

// v_posed of one vertex from the MFMA-ordered three-plane operand images (hi + mid + lo = the fp32 value exactly): 60 lanes take one
// 8-column fragment each.  720 scattered cache lines per vertex - only the overflow path of lbs_fix_process (a full fix-up queue)
// uses it, because it is compact code inside the fused kernel; egx_lbs_fix_kernel reads the vertex-major copy instead.
__device__ __forceinline__ void lbs_fix_blend_planes(const LbsParams& p, int lane, int vt, int row, int bt, int n, float (&v)[3]) {
  v[0] = v[1] = v[2] = 0.f;
  if (lane < 2 * KS3) {
    const int sidx = lane >> 1, hf = lane & 1;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = 0.f;
#pragma unroll
    for (int pl = 2; pl >= 0; --pl) {   // lo + mid first: their sum is exact, then + hi = the fp32 value
      const bf16x8 fr = p.feat3[(((size_t)bt * KS3 + sidx) * 3 + pl) * 64 + hf * 32 + n];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += egx_bf16_to_f32((unsigned short)fr[e]);
    }
    // column 470 (the template's third bf16 term, switched on for the two-plane product) is part of column 469 here
    if (sidx == KS3 - 1 && hf == 0) f[6] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float b[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = 0.f;
#pragma unroll
      for (int pl = 2; pl >= 0; --pl) {
        const bf16x8 br = p.dirs3[((((size_t)vt * KS3 + sidx) * 3 + pl) * 3 + c) * 64 + hf * 32 + row];
#pragma unroll
        for (int e = 0; e < 8; ++e) b[e] += egx_bf16_to_f32((unsigned short)br[e]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[c] = fmaf(f[e], b[e], v[c]);
    }
  }
}

// fp32 re-evaluation of ONE vertex the cheap evaluation of the mixed blend could not decide (see LBS_FIX_SLACK_M): row `row` of vertex
// tile vt for the body in operand slot `slot`.  The whole wave works on it: lane j takes joint j's share of the blend product
// (below), the sums are reduced across the wave, lane jj < JT applies joint jl[jj] of the tile's list (weight Wt[jj * 32 + row]),
// and the trilinear sample decides.  ~70 cache lines per vertex (the first version read the MFMA-ordered operand images: 720
// lines, and 22 000 vertices of a launch with every body inside the obstacle took 330 us).
// Returns -trilinear (wave-uniform); negative = the vertex counts.
template <bool VERTEX_MAJOR, bool MS = false>
__device__ __forceinline__ float lbs_fix_one(const LbsParams& p, int lane, int vt, int row, int slot, int JT, const int* jl, const float* Wt) {
  const int bt = slot >> 5, n = slot & 31;
  const int body = p.agent_of_slot ? p.agent_of_slot[slot / p.fpa] * p.fpa + slot % p.fpa : slot;
  const int ag = body / p.fpa;
  SdfDev sd = p.sdf;   // the body's scene
  if constexpr (MS) {
    int sc;
    lbs_scene_of(p, ag, sc);
    sd = egx_sdf_scene(p.sdf, p.scenes[sc]);
  }
  // v_posed = v_template + shape offsets + pose correctives, in fp32 from the vertex-major bases: lane j owns joint j - it
  // recomputes the joint's rotation from the body's parameter row (the pose kernel's formulas) and multiplies its nine R - I
  // entries with the vertex's nine columns of that joint (36 contiguous bytes per coordinate); lane 0 (the global orientation is
  // not a blend feature) takes the ten shape columns and the template
  float v[3] = {0.f, 0.f, 0.f};
  if constexpr (!VERTEX_MAJOR) {
    lbs_fix_blend_planes(p, lane, vt, row, bt, n, v);
  } else {
    const float* x = p.xb + (size_t)body * EGX_XB_DIM;
    const float* base = p.dirs_rm + ((size_t)vt * 32 + row) * 3 * KDIM;
    if (lane == 0) {
      const float* be = p.betas + (size_t)ag * 10;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float acc = base[c * KDIM + KACT];
        for (int k = 0; k < 10; ++k) acc = fmaf(be[k], base[c * KDIM + k], acc);
        v[c] = acc;
      }
    } else if (lane < NJ && (lane < 22 || lane > 24)) {
      float R[9];
      lbs_joint_rotation(p.pc, x, lane, R);
      const int k0 = 10 + egx_compact_joint(lane) * 9;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 9; ++e) acc = fmaf(R[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f), base[c * KDIM + k0 + e], acc);
        v[c] = acc;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = lbs_wave_sum(v[c]);
  // skinning: one joint of the tile's list per lane
  float o[3] = {0.f, 0.f, 0.f};
  if (lane < JT) {   // JT <= 55 < 64
    const int j = jl[lane] & 0xff;
    const float wv = Wt[lane * 32 + row];
    const f32x4* Aq = p.A4 + ((size_t)bt * NJ + j) * 3 * 32 + n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const f32x4 ar = Aq[a * 32];
      o[a] = wv * fmaf(ar[0], v[0], fmaf(ar[1], v[1], fmaf(ar[2], v[2], ar[3])));
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = lbs_wave_sum(o[a]) + p.xb[(size_t)body * EGX_XB_DIM + a];
  // canonical frame -> world -> voxel coordinates: the folded affine map of the epilogue
  const float kk[3] = {sd.scale * (float)sd.d0 * 0.5f, sd.scale * (float)sd.d1 * 0.5f, sd.scale * (float)sd.d2 * 0.5f};
  const float cc[3] = {sd.cx, sd.cy, sd.cz};
  const float dd[3] = {(float)sd.d0, (float)sd.d1, (float)sd.d2};
  float vox[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float Mw[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) Mw[e] = kk[a] * (p.R0 ? p.R0[(size_t)ag * 9 + a * 3 + e] : ((a == e) ? 1.f : 0.f));
    const float tw = kk[a] * ((p.T0 ? p.T0[(size_t)ag * 3 + a] : 0.f) - cc[a]) + (dd[a] - 1.f) * 0.5f;
    vox[a] = fmaf(Mw[0], o[0], fmaf(Mw[1], o[1], fmaf(Mw[2], o[2], tw)));
  }
  return egx_sdf_neg_trilinear_at(sd, __builtin_amdgcn_fmed3f(vox[0], 0.f, (float)(sd.d0 - 1)), __builtin_amdgcn_fmed3f(vox[1], 0.f, (float)(sd.d1 - 1)),
                                  __builtin_amdgcn_fmed3f(vox[2], 0.f, (float)(sd.d2 - 1)));
}

// What a wave does with the vertices of its item that fell into the band (bit r of s_fixmap[q*32 + n] = row r of the item's
// vertex tile for body (q, n)): they go to the launch's fix-up queue - (vertex tile, row, operand slot) - which
// egx_lbs_fix_kernel works through after the fused kernel, one wave per vertex, thousands of them side by side.  Doing it here
// instead (a whole wave busy for several dependent round trips per vertex while the three other waves of its workgroup wait at
// the next item's barrier) cost 55 us of a 700 us launch for 3 300 vertices; the queue costs one atomic per wave and item
// that has any.  Only when the queue is full are they re-evaluated on the spot.
template <int NB, bool MS = false>
__device__ __forceinline__ void lbs_fix_process(const LbsParams& p, const LbsWave& w, int vt, int bt0, int JT) {
  const int lane = w.lane;
  unsigned mybits = lane < 32 * NB ? w.s_fixmap[lane] : 0u;
  if (mybits != 0u) w.s_fixmap[lane] = 0u;
  unsigned long long pend = __ballot(mybits != 0u);
  // exclusive prefix of the per-lane counts over the (few) lanes that hold any
  const int mine = __popc(mybits);
  int total = 0, my_off = 0;
  for (unsigned long long m = pend; m != 0ull; m &= m - 1) {
    const int sl = __builtin_ctzll(m);
    if (lane == sl) my_off = total;
    total += __builtin_amdgcn_readlane(mine, sl);
  }
  int base = 0;
  const int sq = blockIdx.x % LBS_FIX_NQ;
  int2* q = p.fixq + (size_t)sq * p.fixq_cap;
  if (lane == 0) base = atomicAdd(p.fix_stats + LBS_FIX_CNT0 + 32 * sq, total);
  base = __builtin_amdgcn_readfirstlane(base);
  if (base + total <= p.fixq_cap) {
    const int slot = min((bt0 + (lane >> 5)) * 32 + (lane & 31), p.B - 1);
    for (int k = 0; mybits != 0u; ++k) {
      const int row = __builtin_ctz(mybits);
      mybits &= mybits - 1;
      q[base + my_off + k] = make_int2(vt * 32 + row, slot);
    }
    return;
  }
  // full: what this wave reserved below the capacity is marked void (egx_lbs_fix_kernel skips it), its vertices are done here
  for (int i = base + lane; i < min(base + total, p.fixq_cap); i += 64) q[i] = make_int2(-1, 0);
  while (pend != 0ull) {
    const int sl = __builtin_ctzll(pend);
    pend &= pend - 1;
    unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)mybits, sl);
    const int slot = min((bt0 + (sl >> 5)) * 32 + (sl & 31), p.B - 1);
    while (bits != 0u) {
      const int row = __builtin_ctz(bits);
      bits &= bits - 1;
      const float sv = lbs_fix_one<false, MS>(p, lane, vt, row, slot, JT, w.s_jl, w.s_W);
      if (lane == 0) {
        if (sv < 0.f) atomicAdd(&w.s_cnt[sl], 1);
        atomicAdd(p.fix_stats, 1);
      }
    }
  }
}

// Epilogue of one work item: each lane owns 16 vertices (rows) x 2 bodies (column n of tiles bt0, bt0+1).
template <bool WRITE_VERTS, bool DO_SDF, int RB, int QCAP, int NB = LBS_NB, bool FIX = false, bool MS = false>
__device__ __forceinline__ void lbs_epilogue(const LbsParams& p, LbsWave& w, f32x16 (&acc)[3][NB], int vt, int bt0, int JT, bool fix_on = false) {
  const int lane = w.lane, n = w.n, half = w.half;
  float* s_W = w.s_W; int* s_jl = w.s_jl; int* s_slot = w.s_slot; unsigned* s_masks = w.s_masks; int* s_cnt = w.s_cnt;
  float* lds = w.lds; f32x4* s_queue = w.s_queue;
  int qn = w.qn;
  float tr[NB][3];
  int body[NB];
  bool bvalid[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int slot = (bt0 + q) * 32 + n;     // operand slot; the body it holds (culled launches re-order the agents):
    bvalid[q] = slot < p.B;
    const int sl = bvalid[q] ? slot : p.B - 1;
    body[q] = p.agent_of_slot ? p.agent_of_slot[sl / p.fpa] * p.fpa + sl % p.fpa : sl;
    const int bb = body[q];
    tr[q][0] = p.xb[(size_t)bb * EGX_XB_DIM + 0];
    tr[q][1] = p.xb[(size_t)bb * EGX_XB_DIM + 1];
    tr[q][2] = p.xb[(size_t)bb * EGX_XB_DIM + 2];
  }
  // mixed blend, count-only tiles: |SDF value| below which the cheap evaluation of a body's vertices does not decide = the
  // body's position error bound (pose kernel) x the most the interpolated value can change per metre (aux[3] of the table)
  [[maybe_unused]] float thr[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) thr[q] = 0.f;
  // (set launches: per body tile, with the body's scene, below - the scene is not kept alive across the skinning)
  if constexpr (FIX && DO_SDF && !MS) {
    if (fix_on) {
      const float lip = p.sdf_aux[3];   // steepest slope of the interpolated field, value per metre
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        thr[q] = p.fix_e[min((bt0 + q) * 32 + n, p.B - 1)] * lip;
        w.s_thr[q * 32 + n] = thr[q];   // both lane halves write the same value
      }
    }
  }
  // Skinning walks the tile's joint list: one transform fetch per (joint, body) - prefetched one joint ahead - applied
  // to the lane's 16 vertices with their weights from LDS (o = sum_j w_j (A_j v + t_j); rows whose weights are all zero
  // are skipped in groups of four).  The accumulators already hold v_template + offsets (template column of the GEMM).
  auto sdf_flush = [&](int count) {
    __builtin_amdgcn_wave_barrier();
    for (int base = 0; base < count; base += 64) {
      const int idx = base + lane;
      if (idx < count) {
        const f32x4 e = s_queue[idx];
        int code = __float_as_int(e[3]);   // counter slot | vertex row << 8 (| scene << 16 in set launches)
        float sv;
        if constexpr (MS) {
          sv = egx_sdf_neg_trilinear_at(egx_sdf_scene(p.sdf, p.scenes[code >> 16]), e[0], e[1], e[2]);
          code &= 0xffff;
        } else {
          sv = egx_sdf_neg_trilinear_at(p.sdf, e[0], e[1], e[2]);
        }
        if constexpr (FIX) {
          const float t = fix_on ? w.s_thr[code & 63] : 0.f;
          if (sv < -t) atomicAdd(&s_cnt[code & 63], 1);
          else if (fix_on && sv <= t) {
            const int rr = (code >> 8) & 15;   // accumulator row -> row of the vertex tile
            atomicOr(&w.s_fixmap[code & 63], 1u << ((rr & 3) + 8 * (rr >> 2) + 4 * (code >> 12)));
          }
        } else {
          if (sv < 0.f) atomicAdd(&s_cnt[code & 63], 1);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  // both masks are properties of the TILE: wave-uniform, kept in SGPRs (readfirstlane), so "does this tile hold picked
  // vertices" (8 of 328 tiles) is a scalar branch; the lane's share is one shift by 4 * half, after which every row test is a
  // compile-time bit position.  (Round 4 tested `mask >> row` with row = f(r, half): the compiler hoisted sixteen per-lane
  // `1 << row` constants out of the persistent loop and spilled eleven of them - scratch reloads, each with a vmcnt(0) that
  // drained the transform prefetch.)
  const unsigned pick_mask = p.picked ? (unsigned)__builtin_amdgcn_readfirstlane((int)s_masks[0]) : 0u;
  const unsigned sdf_mask = (unsigned)__builtin_amdgcn_readfirstlane((int)s_masks[1]);
#ifdef EGX_LBS_TIMING
  unsigned long long (&et)[8] = w.et;
#endif
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    [[maybe_unused]] const unsigned long long q0 = LBS_NOW();
    const int ls = lbs_live_slot(bt0 + q, n, p.B);
    const f32x4* Aq = p.A4 + (size_t)(ls >> 5) * NJ * 3 * 32 + (ls & 31);
    // rows are handled in adjacent pairs (r, r+1): the accumulator registers, weights and outputs of a pair are
    // neighbours, so the nine transform FMAs and three weight FMAs map onto packed fp32 instructions
    float o[16][3];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[r][0] = tr[q][0]; o[r][1] = tr[q][1]; o[r][2] = tr[q][2]; }
    f32x4 a0, a1, a2;
    {
      const int j = s_jl[0] & 0xff;   // entries: joint | row-group mask << 8
      a0 = Aq[(j * 3 + 0) * 32]; a1 = Aq[(j * 3 + 1) * 32]; a2 = Aq[(j * 3 + 2) * 32];
    }
    for (int jj = 0; jj < JT; ++jj) {
      const int jn = s_jl[min(jj + 1, JT - 1)] & 0xff;
      const f32x4 n0 = Aq[(jn * 3 + 0) * 32], n1 = Aq[(jn * 3 + 1) * 32], n2 = Aq[(jn * 3 + 2) * 32];
      // which row groups this joint touches: a property of the tile, precomputed at load (round 4 derived it from the weights
      // with four compares, three ORs and a ballot per group, joint and body tile)
      const int gmask = __builtin_amdgcn_readfirstlane(s_jl[jj]) >> 8;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        if (!((gmask >> rg) & 1)) continue;   // scalar branch
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(&s_W[jj * 32 + 8 * rg + 4 * half]);
        // plain v_fma_f32 on purpose (lbs_fma): packed fp32 FMAs beside another wave's MFMAs cost more than they save on
        // gfx950 (MI355X_MICROARCH.md, price of a filler), and the row pairs they need cost two v_mov per operand
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = rg * 4 + e;
          const float vx = acc[0][q][r], vy = acc[1][q][r], vz = acc[2][q][r], wv = w4[e];
          const float px = lbs_fma(a0[0], vx, lbs_fma(a0[1], vy, lbs_fma(a0[2], vz, a0[3])));
          const float py = lbs_fma(a1[0], vx, lbs_fma(a1[1], vy, lbs_fma(a1[2], vz, a1[3])));
          const float pz = lbs_fma(a2[0], vx, lbs_fma(a2[1], vy, lbs_fma(a2[2], vz, a2[3])));
          o[r][0] = lbs_fma(wv, px, o[r][0]);
          o[r][1] = lbs_fma(wv, py, o[r][1]);
          o[r][2] = lbs_fma(wv, pz, o[r][2]);
        }
      }
      a0 = n0; a1 = n1; a2 = n2;
    }
#ifdef EGX_LBS_TIMING
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long q1 = LBS_NOW();
    et[0] += q1 - q0;
#endif
    if (DO_SDF) {
      // Bracket table first (eight independent 8-byte loads per batch).  A vertex the brackets cannot decide needs the
      // eight-corner interpolation; executed in place that would run for the whole wave whenever ONE lane needs it, and
      // with 64 different bodies across the lanes that is almost every row.  Undecided points are therefore appended
      // to a wave-private LDS queue and evaluated densely (64 queued points per pass) by sdf_flush().
      const int ag = body[q] / p.fpa;
      SdfDev sd = p.sdf;   // the body's scene (set launches: its grid, table, center, scale and slope)
      bool sok = true;     // it exists (always, outside set launches)
      [[maybe_unused]] int scn = 0;
      if constexpr (MS) {
        sok = lbs_scene_of(p, ag, scn);
        const SdfSceneDev& sc = p.scenes[scn];
        sd = egx_sdf_scene(p.sdf, sc);
        if constexpr (FIX) {
          if (fix_on) {
            thr[q] = p.fix_e[min((bt0 + q) * 32 + n, p.B - 1)] * sc.slope;
            w.s_thr[q * 32 + n] = thr[q];
          }
        }
      }
      // canonical frame -> world (R0, T0) -> unclamped voxel coordinates ((w - c) scale + 1) d / 2 - 1 / 2 folded into one
      // affine map per body (align_corners=False, utils.py:58-68); the clamp (padding "border") happens in the lookup /
      // before the exact evaluation.  The folded rounding differs from the reference's chain by ~1e-7 relative - far
      // inside the level-set band the counts are compared in.
      float Mw[9], tw[3];
      {
        const float kx = sd.scale * (float)sd.d0 * 0.5f, ky = sd.scale * (float)sd.d1 * 0.5f,
                    kz = sd.scale * (float)sd.d2 * 0.5f;
        const float kk[3] = {kx, ky, kz};
        const float cc[3] = {sd.cx, sd.cy, sd.cz};
        const float dd[3] = {(float)sd.d0, (float)sd.d1, (float)sd.d2};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
          for (int e = 0; e < 3; ++e) Mw[a * 3 + e] = kk[a] * (p.R0 ? p.R0[(size_t)ag * 9 + a * 3 + e] : ((a == e) ? 1.f : 0.f));
          tw[a] = kk[a] * ((p.T0 ? p.T0[(size_t)ag * 3 + a] : 0.f) - cc[a]) + (dd[a] - 1.f) * 0.5f;
        }
      }
      const float hx = (float)(p.sdf.d0 - 1), hy = (float)(p.sdf.d1 - 1), hz = (float)(p.sdf.d2 - 1);
      const unsigned mine = (bvalid[q] && sok) ? (sdf_mask >> (4 * half)) : 0u;  // bit (r&3)+8(r>>2) = this lane's row r
      int cnt = 0;
      // all sixteen bracket lookups of the lane's rows are issued before the first one is used: one L2 round trip per body
      // tile instead of one per batch of RB rows (round 4; the epilogue is a latency chain - two waves per SIMD - and these
      // gathers were four of its eight round trips per item).  The world coordinates are not kept: the rare undecided point
      // recomputes its own (12 FMAs) inside the queue branch.
      auto world = [&](int r, int a) { return fmaf(Mw[a * 3 + 0], o[r][0], fmaf(Mw[a * 3 + 1], o[r][1], fmaf(Mw[a * 3 + 2], o[r][2], tw[a]))); };
      // the bracket lookup wants CELL coordinates r / 4 + 1: the same affine map scaled by 1/4 (exact) with the +1 folded into
      // its constant - three FMAs per point instead of six; a point within round-off of a cell border may land in the
      // neighbouring cell, which egx_sdf_coarse_at_raw already allows for
      float Mc[9], tc[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int e = 0; e < 3; ++e) Mc[a * 3 + e] = 0.25f * Mw[a * 3 + e];
        tc[a] = fmaf(0.25f, tw[a], 1.f);
      }
      auto cell = [&](int r, int a) { return fmaf(Mc[a * 3 + 0], o[r][0], fmaf(Mc[a * 3 + 1], o[r][1], fmaf(Mc[a * 3 + 2], o[r][2], tc[a]))); };
      // rows per lookup burst: the vertex-writing variant has no registers to spare, nor has the mixed blend's set launch (its body's
      // table pointer is live beside the accumulators; this path takes only its picked and long-list tiles, 27 of 328)
      constexpr int LB = WRITE_VERTS ? RB : ((MS && FIX) ? 8 : 16);
#pragma unroll
      for (int rb0 = 0; rb0 < 16; rb0 += LB) {
      float2 mm[LB];
#pragma unroll
      for (int r = rb0; r < rb0 + LB; ++r) mm[r - rb0] = egx_sdf_coarse_at_cell(sd, cell(r, 0), cell(r, 1), cell(r, 2));
#pragma unroll
      for (int r0 = rb0; r0 < rb0 + LB; r0 += RB) {
        if (qn + RB * 64 > QCAP) { sdf_flush(qn); qn = 0; }  // room for one batch: RB rows x 64 lanes
#pragma unroll
        for (int r = r0; r < r0 + RB; ++r) {
          const bool on = (mine >> ((r & 3) + 8 * (r >> 2))) & 1u;
          const bool inside = mm[r - rb0].x > thr[q];
          cnt += (on && inside) ? 1 : 0;
          const bool und = on && !inside && !(mm[r - rb0].y < -thr[q]);
          const unsigned long long bm = __ballot(und);
          if (bm != 0) {
            const int pos = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u));
            if (und) {
              // counter slot | accumulator row r << 8 | lane half << 12, formed here (as loop invariants the sixteen per-lane
              // codes of a body tile would be kept alive across the whole item)
              int ln = lane;
              asm volatile("" : "+v"(ln));
              s_queue[pos] = f32x4{__builtin_amdgcn_fmed3f(world(r, 0), 0.f, hx), __builtin_amdgcn_fmed3f(world(r, 1), 0.f, hy),
                                   __builtin_amdgcn_fmed3f(world(r, 2), 0.f, hz),
                                   __int_as_float((q * 32 + (ln & 31)) | (r << 8) | ((ln >> 5) << 12) | (MS ? scn << 16 : 0))};
            }
            qn += __popcll(bm);
          }
        }
      }
      }
      if (cnt != 0) {
        int nn = n;                       // address formed here (see run_item: no loop-invariant per-lane address to keep alive)
        asm volatile("" : "+v"(nn));
        atomicAdd(&s_cnt[q * 32 + nn], cnt);
      }
      if (WRITE_VERTS) { sdf_flush(qn); qn = 0; }  // the queue shares its LDS with the vertex transpose buffer
    }
#ifdef EGX_LBS_TIMING
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long q2 = LBS_NOW();
    et[1] += q2 - q1;
#endif
    if (pick_mask != 0) {   // scalar branch
      const unsigned pmine = bvalid[q] ? (pick_mask >> (4 * half)) : 0u;   // bit (r&3)+8(r>>2) = this lane's row r
      const int* slot_h = s_slot + 4 * half;
      float* pbase = p.picked + (size_t)body[q] * p.NP * 3;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if ((pmine >> ((r & 3) + 8 * (r >> 2))) & 1u) {
          float* op = pbase + slot_h[(r & 3) + 8 * (r >> 2)] * 3;
          op[0] = o[r][0]; op[1] = o[r][1]; op[2] = o[r][2];
        }
      }
    }
    if (WRITE_VERTS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        lds[n * 97 + row * 3 + 0] = o[r][0];
        lds[n * 97 + row * 3 + 1] = o[r][1];
        lds[n * 97 + row * 3 + 2] = o[r][2];
      }
    }
    if (WRITE_VERTS) {
      // transpose through LDS so that one wave instruction writes whole vertices of ONE body (the rows of a tile are
      // in the joint-sorted order: each lands at its original vertex id; wave-private LDS region, DS ops of one wave
      // execute in order, no barrier needed)
      int dst[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int f = lane + 64 * u;  // f = row * 3 + coordinate, 96 values per body
        const int vo = (f < 96) ? p.vorig[vt * 32 + f / 3] : -1;
        dst[u] = (vo >= 0) ? vo * 3 + f % 3 : -1;
      }
      for (int bi = 0; bi < 32; ++bi) {
        const int bd = (bt0 + q) * 32 + bi;
        if (bd >= p.B) break;
        float* o = p.verts + (size_t)bd * p.V * 3;
#pragma unroll
        for (int u = 0; u < 2; ++u)
          if (dst[u] >= 0) o[dst[u]] = lds[bi * 97 + lane + 64 * u];
      }
    }
  }
#ifdef EGX_LBS_TIMING
  const unsigned long long f0 = LBS_NOW();
#endif
  if (DO_SDF) {
    if (!WRITE_VERTS) { sdf_flush(qn); qn = 0; }
    __builtin_amdgcn_wave_barrier();
    if constexpr (FIX) {
      if (fix_on) {   // wave-uniform
        const unsigned fb = lane < 32 * NB ? w.s_fixmap[lane] : 0u;
        if (__ballot(fb != 0u) != 0ull) lbs_fix_process<NB, MS>(p, w, vt, bt0, JT);
        __builtin_amdgcn_wave_barrier();
      }
    }
    const int c = lane < 32 * NB ? s_cnt[lane] : 0;   // lane = q*32 + n: one global atomic per body and item
    if (lane < 32 * NB) s_cnt[lane] = 0;
    const int sd = (bt0 + (lane >> 5)) * 32 + (lane & 31);
    if (c != 0 && sd < p.B && lane < 32 * NB) {
      const int bd = p.agent_of_slot ? p.agent_of_slot[sd / p.fpa] * p.fpa + sd % p.fpa : sd;
      atomicAdd(p.pene + bd, c);
    }
    __builtin_amdgcn_wave_barrier();
  }
#ifdef EGX_LBS_TIMING
  __builtin_amdgcn_sched_barrier(0);
  et[2] += LBS_NOW() - f0;
  et[3] += 1;
#endif
  w.qn = qn;
}
