// ------------------------------------------------------------------------------------------------
// kernel 2b: the same work item with the blend GEMM as a 3-term bf16 split (see KS3 above).
// Workgroup = 4 waves = one vertex tile x 256 bodies; the bases of a stage (2 k-steps x 3 planes x 3 coordinates = 18
// pieces of 1 KiB) are fetched once per workgroup, parked in LDS (double buffered, one barrier per stage) and read back
// by all four waves; each wave fetches its own feature pieces (12 KiB per stage) into registers.  Loads are issued as a
// burst and waited for before the stage's 72 MFMAs (no VMEM in flight under MFMA, scripts/ubench/mfma_bf16.hip); the
// second workgroup of the CU covers the gap, and - unlike the fp32 MFMA, which shares the fp32 VALU lanes - the bf16
// matrix pipe runs concurrently with the other workgroup's VALU epilogue.
// ------------------------------------------------------------------------------------------------
#include <algorithm>
#include <cstdlib>

#include "lbs_epilogue.h"

#ifdef EGX_LBS_TIMING
// development build only (make CXXFLAGS+=-DEGX_LBS_TIMING): cycle totals of the phases of the bf16x3 stage loop.  Without relocatable
// device code a __device__ variable belongs to one translation unit: it sits with the kernel that writes it and the call that reads it.
__device__ unsigned long long g_lbs_t[16];
#endif

#define LBS_MFMA_RESULT_WAIT()                   \
  do {                                           \
    __builtin_amdgcn_sched_barrier(0);           \
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0);           \
  } while (0)

// Epilogue of a COUNT-ONLY tile of the mixed blend (mode 3; a tile after the ones that hold picked vertices, joint list of at most
// eight): skinning on the matrix pipe, straight into SDF-cell coordinates.
//   o_cell[v, body] = cinit[body] + sum_j W[v, j] (A'_j [v_posed; 1]),   A'_j = Mc A_j   (pose kernel: skinB, cinit)
// is evaluated as T = W x A' - twelve 32 x 32 outputs per 32-body tile, one per entry (a, c) of the 3 x 4 transform, K = the eight
// joints of the tile's list x the two planes of A' (see SKIN_BT_BYTES), two MFMAs each - followed by
// o[a] = T[a][0] x + T[a][1] y + T[a][2] z + T[a][3] on the accumulators of the blend GEMM, which already hold (x, y, z) in the
// same lane layout: 9 FMAs per (vertex, body) instead of 12 per (vertex, body, joint), and no canonical -> cell map (9 more)
// afterwards.  The operands of a body tile arrive in ONE burst (24 bytes per joint and lane, joint-major) and are turned into
// MFMA operands (entry-major, eight joints each) by 48 v_perm_b32: one L2 round trip per body tile instead of one per joint.
// What it costs: 24 MFMAs per body tile on a matrix pipe that was 23 % busy, and a position error of up to LBS_SKIN_ERR (|v| + |t|),
// which the fix-up band absorbs - the result only classifies, lbs_fix_process decides the close calls.
template <int RB, int QCAP, int NB, bool MS = false>
__device__ __forceinline__ void lbs_epilogue_cell(const LbsParams& p, LbsWave& w, f32x16 (&acc)[3][NB], int vt, int bt0, int JT) {
  int lane = w.lane;
  asm volatile("" : "+v"(lane));   // per-lane operand addresses are formed per item (not kept alive as invariants of the persistent loop)
  const int n = lane & 31, half = lane >> 5;
  int* s_cnt = w.s_cnt;
  f32x4* s_queue = w.s_queue;
  int qn = w.qn;
  const unsigned sdf_mask = (unsigned)__builtin_amdgcn_readfirstlane((int)w.s_masks[1]);
  const int ks0 = __builtin_amdgcn_readfirstlane(p.skin_ks_off[vt]);   // JT <= 8 here: one k-step (the caller sends longer lists to the VALU epilogue)
  [[maybe_unused]] float lip = 0.f;   // steepest slope of the interpolated field, value per metre (set launches: per body, below)
  if constexpr (!MS) lip = p.sdf_aux[3];
  const float hx = (float)(p.sdf.d0 - 1), hy = (float)(p.sdf.d1 - 1), hz = (float)(p.sdf.d2 - 1);
  auto sdf_flush = [&](int count) {
    __builtin_amdgcn_wave_barrier();
    for (int base = 0; base < count; base += 64) {
      const int idx = base + lane;
      if (idx < count) {
        const f32x4 e = s_queue[idx];
        int code = __float_as_int(e[3]);   // counter slot | accumulator row << 8 | lane half << 12 (| scene << 16 in set launches)
        float sv;
        if constexpr (MS) {
          sv = egx_sdf_neg_trilinear_at(egx_sdf_scene(p.sdf, p.scenes[code >> 16]), e[0], e[1], e[2]);
          code &= 0xffff;
        } else {
          sv = egx_sdf_neg_trilinear_at(p.sdf, e[0], e[1], e[2]);
        }
        const float t = w.s_thr[code & 63];
        if (sv < -t) atomicAdd(&s_cnt[code & 63], 1);
        else if (sv <= t) {
          const int rr = (code >> 8) & 15;
          atomicOr(&w.s_fixmap[code & 63], 1u << ((rr & 3) + 8 * (rr >> 2) + 4 * (code >> 12)));
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  // two 16-bit entries of neighbouring joints -> one operand register: v_perm_b32 picks the low (even entry) or high halves
  auto pack2 = [](unsigned hi_joint, unsigned lo_joint, int odd) {
    return odd ? __builtin_amdgcn_perm(hi_joint, lo_joint, 0x07060302u) : __builtin_amdgcn_perm(hi_joint, lo_joint, 0x05040100u);
  };
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  // the tile's joint list (LDS, published by the blend's barriers) -> one register, read out lane by lane below: a load per
  // entry in front of its records would make every body tile a chain of JT round trips again
  const int jl_v = w.s_jl[min(lane, JT - 1)] & 0xff;
  // the tile's weight operands: once per item
  const bf16x8 W0 = p.skinW[((size_t)ks0 * 2 + 0) * 64 + lane], W1 = p.skinW[((size_t)ks0 * 2 + 1) * 64 + lane];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int slot = (bt0 + q) * 32 + n;
    const bool bvalid = slot < p.B;
    const f32x4 ci = p.cinit[bvalid ? slot : p.B - 1];
    [[maybe_unused]] float fe = 0.f;
    if constexpr (!MS) fe = p.fix_e[bvalid ? slot : p.B - 1];   // requested here, used after the skinning (set launches: below)
    // this lane's records: plane = lane half, body column n; record of joint j at index j * 64
    const int ls = lbs_live_slot(bt0 + q, n, p.B);
    const char* tile_base = reinterpret_cast<const char*>(p.skinB) + (size_t)(ls >> 5) * SKIN_BT_BYTES;
    const u32x4* recA = reinterpret_cast<const u32x4*>(tile_base) + half * 32 + (ls & 31);
    const u32x2* recB = reinterpret_cast<const u32x2*>(tile_base + (size_t)SKIN_BT_A * 16) + half * 32 + (ls & 31);
    float o[16][3];
    {
      // all twelve entries of the (up to) eight joints in ONE burst: 16 + 8 bytes per joint and lane
      u32x4 RA[8];
      u32x2 RC[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (e < JT) {   // scalar branch
          const int j = __builtin_amdgcn_readlane(jl_v, e);
          RA[e] = recA[j * 64];
          RC[e] = recB[j * 64];
        } else {        // the weights of the unused slots are zero: any finite operand does
          RA[e] = u32x4{0u, 0u, 0u, 0u};
          RC[e] = u32x2{0u, 0u};
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      // records (joint-major) -> operands (entry-major, eight joints per operand): all twelve now, so that the 48 record registers
      // are free before the first accumulators are
      bf16x8 Bop[12];
#pragma unroll
      for (int cc = 0; cc < 12; ++cc) {
        u32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          v[i] = cc < 8 ? pack2(RA[2 * i + 1][cc >> 1], RA[2 * i][cc >> 1], cc & 1) : pack2(RC[2 * i + 1][(cc - 8) >> 1], RC[2 * i][(cc - 8) >> 1], cc & 1);
        Bop[cc] = __builtin_bit_cast(bf16x8, v);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        // two entries of the row at a time (32 accumulator registers live instead of 64): (translation, x) then (y, z);
        // W_mid A'_hi first (the small term), then W_hi (A'_hi + A'_mid)
        f32x16 Ta, Tb;
#pragma unroll
        for (int r = 0; r < 16; ++r) { Ta[r] = ci[a]; Tb[r] = 0.f; }
        Ta = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1, Bop[a * 4 + 3], Ta, 0, 0, 0);
        Tb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1, Bop[a * 4 + 0], Tb, 0, 0, 0);
        Ta = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W0, Bop[a * 4 + 3], Ta, 0, 0, 0);
        Tb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W0, Bop[a * 4 + 0], Tb, 0, 0, 0);
        float oa[16];
#pragma unroll
        // The FMAs below are inline asm (lbs_fma: see there), which the compiler's hazard recogniser does not look into: the wait
        // states between an MFMA and a VALU read of its result (software-managed on CDNA: up to 19 for a 16-pass MFMA) are put
        // here by hand.  Without them the FMAs read accumulators the matrix pipe is still writing.
        LBS_MFMA_RESULT_WAIT();
        for (int r = 0; r < 16; ++r) oa[r] = lbs_fma(Tb[r], acc[0][q][r], Ta[r]);
#pragma unroll
        for (int r = 0; r < 16; ++r) { Ta[r] = 0.f; Tb[r] = 0.f; }
        Ta = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1, Bop[a * 4 + 1], Ta, 0, 0, 0);
        Tb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1, Bop[a * 4 + 2], Tb, 0, 0, 0);
        Ta = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W0, Bop[a * 4 + 1], Ta, 0, 0, 0);
        Tb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W0, Bop[a * 4 + 2], Tb, 0, 0, 0);
#pragma unroll
        LBS_MFMA_RESULT_WAIT();
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r][a] = lbs_fma(Ta[r], acc[1][q][r], lbs_fma(Tb[r], acc[2][q][r], oa[r]));
      }
    }
    // SDF: bracket lookups of all sixteen rows in one burst (cell coordinates are what the skinning produced), decisions with the
    // body's band, undecided points to the wave's queue as clamped voxel coordinates 4 (cell - 1).  Set launches look the body's
    // scene up here, after the skinning: its table pointer is not kept alive across the MFMAs
    bool sok = true;   // the body's scene exists (always, outside set launches)
    [[maybe_unused]] int scn = 0;
    SdfDev sd = p.sdf;
    [[maybe_unused]] float lip_q = lip;
    if constexpr (MS) {
      sok = lbs_scene_of(p, (bvalid ? slot : p.B - 1) / p.fpa, scn);
      const SdfSceneDev& sc = p.scenes[scn];
      sd = egx_sdf_scene(p.sdf, sc);
      lip_q = sc.slope;
      fe = p.fix_e[bvalid ? slot : p.B - 1];
    }
    const unsigned mine = (bvalid && sok) ? (sdf_mask >> (4 * half)) : 0u;
    int cnt = 0;
    float2 mm[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) mm[r] = egx_sdf_coarse_at_cell(sd, o[r][0], o[r][1], o[r][2]);
    const float thr = fe * lip_q;
    w.s_thr[q * 32 + n] = thr;   // both lane halves write the same value
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += RB) {
      if (qn + RB * 64 > QCAP) { sdf_flush(qn); qn = 0; }
#pragma unroll
      for (int r = r0; r < r0 + RB; ++r) {
        const bool on = (mine >> ((r & 3) + 8 * (r >> 2))) & 1u;
        const bool inside = mm[r].x > thr;
        cnt += (on && inside) ? 1 : 0;
        const bool und = on && !inside && !(mm[r].y < -thr);
        const unsigned long long bm = __ballot(und);
        if (bm != 0) {
          const int pos = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u));
          if (und) {
            int ln = lane;
            asm volatile("" : "+v"(ln));
            s_queue[pos] = f32x4{__builtin_amdgcn_fmed3f(fmaf(4.f, o[r][0], -4.f), 0.f, hx), __builtin_amdgcn_fmed3f(fmaf(4.f, o[r][1], -4.f), 0.f, hy),
                                 __builtin_amdgcn_fmed3f(fmaf(4.f, o[r][2], -4.f), 0.f, hz),
                                 __int_as_float((q * 32 + (ln & 31)) | (r << 8) | ((ln >> 5) << 12) | (MS ? scn << 16 : 0))};
          }
          qn += __popcll(bm);
        }
      }
    }
    if (cnt != 0) {
      int nn = n;
      asm volatile("" : "+v"(nn));
      atomicAdd(&s_cnt[q * 32 + nn], cnt);
    }
  }
  sdf_flush(qn);
  qn = 0;
  __builtin_amdgcn_wave_barrier();
  {
    const unsigned fb = lane < 32 * NB ? w.s_fixmap[lane] : 0u;
    if (__ballot(fb != 0u) != 0ull) lbs_fix_process<NB, MS>(p, w, vt, bt0, JT);
    __builtin_amdgcn_wave_barrier();
  }
  const int c = lane < 32 * NB ? s_cnt[lane] : 0;   // lane = q*32 + n: one global atomic per body and item
  if (lane < 32 * NB) s_cnt[lane] = 0;
  const int sd = (bt0 + (lane >> 5)) * 32 + (lane & 31);
  if (c != 0 && sd < p.B && lane < 32 * NB) {
    const int bd = p.agent_of_slot ? p.agent_of_slot[sd / p.fpa] * p.fpa + sd % p.fpa : sd;
    atomicAdd(p.pene + bd, c);
  }
  __builtin_amdgcn_wave_barrier();
  w.qn = qn;
}

template <int NPL>
struct Wg4Cfg {
  static constexpr int STAGE_KS = NPL == 3 ? 2 : 3;          // k-steps per stage: 72 / 54 MFMAs per wave and stage
  static constexpr int STAGE_PIECES = STAGE_KS * NPL * 3;    // 1 KiB base pieces per stage
  static constexpr int STAGES = KS3 / STAGE_KS;
  static_assert(KS3 % STAGE_KS == 0, "stages cover K exactly");
};
constexpr int LBS3_SHARED_BYTES = 2 * 18 * 1024 + 7424;                // stage ring (18 pieces in either mode) + tile metadata
static_assert(Wg4Cfg<3>::STAGE_PIECES <= 18 && Wg4Cfg<2>::STAGE_PIECES <= 18, "stage ring");
constexpr int LBS3_RB = 4;                                             // SDF rows per bracket batch
constexpr int LBS3_QCAP = LBS3_RB * 64 + 64;
// the small wave tile runs THREE workgroups per CU and must stay below round 5's 53.5 KB of LDS per workgroup to do so (with the
// fix-up bitmap and thresholds added, 54.0 KB, the launch lost the third workgroup: +45 % at every size): its queue gives up 32 entries
template <int NBW> constexpr int lbs3_qcap() { return NBW == 1 ? LBS3_RB * 64 + 32 : LBS3_QCAP; }
// per-wave LDS of the fused3 kernels: penetration counters, fix-up bitmap, fix-up thresholds (32 x NB entries each), queue
template <int NBW> constexpr int lbs3_wave_bytes() { return 3 * 128 * NBW + lbs3_qcap<NBW>() * 16; }

template <int NPL>
__device__ __forceinline__ void lbs_blend_split(const LbsParams& p, f32x16 (&acc)[3][LBS_NB], int vt, int bt0, int lane, int wave,
                                                bf16x8* sA, unsigned long long* tacc) {
  using Cfg = Wg4Cfg<NPL>;
  constexpr int NB = LBS_NB, SKS = Cfg::STAGE_KS, SP = Cfg::STAGE_PIECES;
  asm volatile("" : "+v"(lane));   // per-lane operand addresses are formed per item (not kept alive as invariants of the persistent loop)
  const bf16x8* dpv = p.dirs3 + (size_t)vt * KS3 * 9 * 64 + lane;  // piece (s, plane, coord) at ((s*3 + plane)*3 + coord)*64
  const bf16x8* fq[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int ls = lbs_live_slot(bt0 + q, lane & 31, p.B);
    fq[q] = p.feat3 + (size_t)(ls >> 5) * KS3 * 3 * 64 + (lane & 32) + (ls & 31);
  }
  for (int st = 0; st < Cfg::STAGES; ++st) {
    // burst: this wave's share of the stage's base pieces + its own feature pieces
    constexpr int NGA = (SP + 3) / 4;
    bf16x8 ga[NGA], b[SKS][NPL][NB];
    [[maybe_unused]] const unsigned long long t0 = LBS_NOW();
#pragma unroll
    for (int i = 0; i < NGA; ++i) {
      const int piece = wave + 4 * i;                 // (ks, plane, coord) of the stage, planes 0..NPL-1 only
      if (piece < SP) ga[i] = dpv[(size_t)((st * SKS + piece / (NPL * 3)) * 9 + piece % (NPL * 3)) * 64];
    }
#pragma unroll
    for (int ks = 0; ks < SKS; ++ks)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int q = 0; q < NB; ++q) b[ks][pl][q] = fq[q][((st * SKS + ks) * 3 + pl) * 64];
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    [[maybe_unused]] const unsigned long long t1 = LBS_NOW();
    bf16x8* buf = sA + (st & 1) * 18 * 64;
#pragma unroll
    for (int i = 0; i < NGA; ++i) {
      const int piece = wave + 4 * i;
      if (piece < SP) buf[piece * 64 + lane] = ga[i];
    }
    __syncthreads();  // stage visible; also: everyone is done reading the other buffer's previous contents
    [[maybe_unused]] const unsigned long long t2 = LBS_NOW();
#pragma unroll
    for (int ks = 0; ks < SKS; ++ks) {
      bf16x8 a[NPL][3];  // [plane][coord]
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[pl][c] = buf[((ks * NPL + pl) * 3 + c) * 64 + lane];
      // product-major order: consecutive MFMAs go to different accumulator tuples, so no MFMA waits for the previous
      // one's result (small partial products first)
      constexpr int NPROD = NPL == 3 ? 6 : 3;
#pragma unroll
      for (int pr = 0; pr < NPROD; ++pr) {
        int pa, pb;
        if (NPL == 3) {
          pa = (pr == 0) ? 1 : (pr == 1) ? 0 : (pr == 2) ? 2 : (pr == 3) ? 0 : (pr == 4) ? 1 : 0;
          pb = (pr == 0) ? 1 : (pr == 1) ? 2 : (pr == 2) ? 0 : (pr == 3) ? 1 : (pr == 4) ? 0 : 0;
        } else {
          pa = (pr == 0) ? 0 : (pr == 1) ? 1 : 0;
          pb = (pr == 0) ? 1 : (pr == 1) ? 0 : 0;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int q = 0; q < NB; ++q)
            acc[c][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa][c], b[ks][pb][q], acc[c][q], 0, 0, 0);
      }
    }
#ifdef EGX_LBS_TIMING
    {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long t3 = LBS_NOW();
      LBS_T(0, t1 - t0); LBS_T(1, t2 - t1); LBS_T(2, t3 - t2); LBS_T(3, 1);
    }
#endif
  }
}

// Mixed blend (mode 3, see M4_BASE_PIECES): nine stages per item - the precise k-step 0, seven stages of four fp16 k-steps, the
// precise k-step 29 - each a burst (this wave's share of the stage's base pieces + its own feature pieces), s_waitcnt, the base
// pieces through the two-deep LDS ring, one barrier, then only MFMAs (the in-flight-load hazard of lbs_blend_f32).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int M4_RING_PIECES = 3 * M4_FKS;      // 12 KiB per ring slot (a precise stage uses 6)
static_assert(28 % M4_FKS == 0, "fp16 stages cover k-steps 1..28 exactly");

// Operand registers of one stage: this wave's share of the stage's base pieces (on their way to the LDS ring) and its own
// feature pieces.
template <int NB>
struct M4Regs {
  bf16x8 ga[(3 * M4_FKS + 3) / 4];
  bf16x8 b[M4_FKS][NB];
};
constexpr int M4_STAGES = 2 + 28 / M4_FKS;     // precise k-step 0, the fp16 stages, precise k-step 29
__device__ __forceinline__ constexpr bool m4_precise(int st) { return st == 0 || st == M4_STAGES - 1; }
__device__ __forceinline__ constexpr int m4_base0(int st) { return st == 0 ? 0 : (st == M4_STAGES - 1 ? 90 : 6 + (st - 1) * 3 * M4_FKS); }
__device__ __forceinline__ constexpr int m4_feat0(int st) { return st == 0 ? 0 : (st == M4_STAGES - 1 ? 30 : 2 + (st - 1) * M4_FKS); }

// The nine stages of an item as a software pipeline of depth one: the burst of stage st + 1 is issued as soon as stage st's
// operands have arrived - before stage st's barrier and MFMAs - so a stage costs max(operand latency, LDS + barrier + MFMAs)
// instead of their sum.  (The in-flight-load hazard of lbs_blend_f32 halves the MFMA rate of this wave meanwhile; here the
// MFMAs are a quarter of the GEMM half - 204 per item - and the operand latency, bases streaming from the Infinity Cache, is
// what the half waits for: 0.414 ms with the epilogue skipped against 0.10 ms of matrix time, profiles/r05_lbs_mixed.md.)
template <int NB>
__device__ __forceinline__ void lbs_blend_mixed(const LbsParams& p, f32x16 (&acc)[3][NB], int vt, int bt0, int lane, int wave, bf16x8* sA,
                                                unsigned long long* tacc) {
  asm volatile("" : "+v"(lane));   // per-lane operand addresses are formed per item
  const bf16x8* dpv = p.dirs4 + (size_t)vt * M4_BASE_PIECES * 64 + lane;
  const bf16x8* fq[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int ls = lbs_live_slot(bt0 + q, lane & 31, p.B);
    fq[q] = p.feat4 + (size_t)(ls >> 5) * M4_FEAT_PIECES * 64 + (lane & 32) + (ls & 31);
  }
  M4Regs<NB> R[2];
  auto issue = [&](M4Regs<NB>& r, int st) {
    const int np = m4_precise(st) ? 6 : 3 * M4_FKS, nf = m4_precise(st) ? 2 : M4_FKS;
#pragma unroll
    for (int i = 0; i < (3 * M4_FKS + 3) / 4; ++i) {
      const int piece = wave + 4 * i;
      if (piece < np) r.ga[i] = dpv[(size_t)(m4_base0(st) + piece) * 64];
    }
#pragma unroll
    for (int f = 0; f < M4_FKS; ++f)
      if (f < nf) {
#pragma unroll
        for (int q = 0; q < NB; ++q) r.b[f][q] = fq[q][(size_t)(m4_feat0(st) + f) * 64];
      }
  };
  issue(R[0], 0);
#pragma unroll
  for (int st = 0; st < M4_STAGES; ++st) {
    M4Regs<NB>& r = R[st & 1];
    bf16x8* buf = sA + (st & 1) * M4_RING_PIECES * 64;
    [[maybe_unused]] const unsigned long long t0 = LBS_NOW();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // stage st's operands (issued a stage ago)
    __builtin_amdgcn_sched_barrier(0);
    [[maybe_unused]] const unsigned long long t1 = LBS_NOW();
    const int np = m4_precise(st) ? 6 : 3 * M4_FKS;
#pragma unroll
    for (int i = 0; i < (3 * M4_FKS + 3) / 4; ++i) {
      const int piece = wave + 4 * i;
      if (piece < np) buf[piece * 64 + lane] = r.ga[i];
    }
    if (st + 1 < M4_STAGES) issue(R[(st + 1) & 1], st + 1);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // stage visible; also: everyone is done reading the other ring slot's previous contents
    [[maybe_unused]] const unsigned long long t2 = LBS_NOW();
    if (m4_precise(st)) {
      bf16x8 a[2][3];   // [plane][coord]
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[pl][c] = buf[(pl * 3 + c) * 64 + lane];
#pragma unroll
      for (int pr = 0; pr < 3; ++pr) {   // hi.mid, mid.hi, hi.hi: small partial products first, product-major
        const int pa = (pr == 1) ? 1 : 0, pb = (pr == 0) ? 1 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int q = 0; q < NB; ++q)
            acc[c][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa][c], r.b[pb][q], acc[c][q], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < M4_FKS; ++ks) {
        bf16x8 a[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = buf[(ks * 3 + c) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int q = 0; q < NB; ++q)
            acc[c][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[c]), __builtin_bit_cast(f16x8, r.b[ks][q]),
                                                               acc[c][q], 0, 0, 0);
      }
    }
#ifdef EGX_LBS_TIMING
    {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long t3 = LBS_NOW();
      LBS_T(0, t1 - t0); LBS_T(1, t2 - t1); LBS_T(2, t3 - t2); LBS_T(3, 1);
    }
#endif
  }
}

// The two-plane split (mode 2 arithmetic) for the tiles that hold picked vertices, on the small LDS ring of the three-workgroups-
// per-CU kernel: stages of two k-steps (12 base pieces: 2 k-steps x 2 planes x 3 coordinates), burst -> wait -> ring -> barrier ->
// 3 products per k-step.  8 of ~320 tiles: simple, not pipelined.
template <int NB>
__device__ __forceinline__ void lbs_blend_split2_small(const LbsParams& p, f32x16 (&acc)[3][NB], int vt, int bt0, int lane, int wave,
                                                       bf16x8* sA) {
  asm volatile("" : "+v"(lane));
  const bf16x8* dpv = p.dirs3 + (size_t)vt * KS3 * 9 * 64 + lane;  // piece (s, plane, coord) at ((s*3 + plane)*3 + coord)*64
  const bf16x8* fq[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int ls = lbs_live_slot(bt0 + q, lane & 31, p.B);
    fq[q] = p.feat3 + (size_t)(ls >> 5) * KS3 * 3 * 64 + (lane & 32) + (ls & 31);
  }
  static_assert(KS3 % 2 == 0, "stages of two k-steps");
  for (int st = 0; st < KS3 / 2; ++st) {
    bf16x8 ga[3], b[2][2][NB];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int piece = wave + 4 * i;                 // (ks, plane, coord) of the stage: ks = piece / 6, plane = piece % 6 / 3
      ga[i] = dpv[(size_t)((st * 2 + piece / 6) * 9 + (piece % 6)) * 64];
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int q = 0; q < NB; ++q) b[ks][pl][q] = fq[q][((st * 2 + ks) * 3 + pl) * 64];
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    bf16x8* buf = sA + (st & 1) * M4_RING_PIECES * 64;
#pragma unroll
    for (int i = 0; i < 3; ++i) buf[(wave + 4 * i) * 64 + lane] = ga[i];
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[2][3];
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[pl][c] = buf[((ks * 2 + pl) * 3 + c) * 64 + lane];
#pragma unroll
      for (int pr = 0; pr < 3; ++pr) {
        const int pa = (pr == 1) ? 1 : 0, pb = (pr == 0) ? 1 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int q = 0; q < NB; ++q)
            acc[c][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa][c], b[ks][pb][q], acc[c][q], 0, 0, 0);
      }
    }
  }
}

// LDS of the fused3 kernels: [operand ring][tile metadata 7424 B][4 x (counters 256 B + queue)].  NBW = 32-body tiles per wave:
// 2 = the round-2..4 shape (a workgroup item = 32 vertices x 256 bodies, two workgroups per CU, 256 registers per wave);
// 1 (mixed blend only, round 5) = 32 vertices x 128 bodies, THREE workgroups per CU: 48 accumulators instead of 96 fit a wave in
// 168 registers, and the third wave per SIMD is what the latency chain of this kernel was missing - one workgroup per CU runs
// the launch in 1.07 ms, two in 0.70 (profiles/r05_lbs_mixed.md section 5).
template <int NBW> constexpr int lbs3_ring_bytes() { return NBW == 1 ? 2 * M4_RING_PIECES * 1024 : 2 * 18 * 1024; }
template <int NBW> constexpr size_t lbs3_lds_bytes() { return (size_t)lbs3_ring_bytes<NBW>() + 7424 + 4 * lbs3_wave_bytes<NBW>(); }
static_assert(lbs3_lds_bytes<1>() <= 53504, "three workgroups of the small wave tile share a CU's LDS: not above round 5's size");

template <int NPL, bool DO_SDF, int NBW = LBS_NB, bool MS = false>
__global__ __launch_bounds__(256, NBW == 1 ? 3 : 2) void egx_lbs_fused3_kernel(LbsParams p) {
  constexpr int NB = NBW;
  static_assert(NBW == LBS_NB || NPL == 4, "the small wave tile exists for the mixed blend only");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave id: an SGPR
  bf16x8* sA = reinterpret_cast<bf16x8*>(smem_raw);
  char* meta = smem_raw + lbs3_ring_bytes<NBW>();
  char* my = meta + 7424 + wave * lbs3_wave_bytes<NBW>();
  LbsWave w;
  w.lane = lane; w.n = lane & 31; w.half = lane >> 5;
  w.s_W = reinterpret_cast<float*>(meta);                    // tile metadata is shared by the four waves here
  w.s_jl = reinterpret_cast<int*>(meta + NJ * 32 * 4);
  w.s_slot = w.s_jl + 56;
  w.s_masks = reinterpret_cast<unsigned*>(w.s_slot + 32);
  w.s_cnt = reinterpret_cast<int*>(my);
  w.s_fixmap = reinterpret_cast<unsigned*>(my + 128 * NBW);
  w.s_thr = reinterpret_cast<float*>(my + 256 * NBW);
  w.s_queue = reinterpret_cast<f32x4*>(my + 384 * NBW);
  w.lds = nullptr;
  w.qn = 0;
  if (lane < 32 * NBW) { w.s_cnt[lane] = 0; w.s_fixmap[lane] = 0u; }
  // Work partition over the XCDs (blocks are dealt to them round-robin).  Either every XCD owns a chunk of BODY GROUPS and
  // all vertex tiles (its bodies' features / transforms stay in its L2 and the bases stream through once per block of groups)
  // or a chunk of VERTEX TILES and all groups (it streams an eighth of the bases once per block; every XCD reads all
  // features).  The bases traffic is the same either way; what differs is the balance: 20 groups (256 agents) deal 3 / 2 over
  // the XCDs, 10 groups (128) deal 2 / 1, 5 groups (64 agents, the 8-way split) leave three XCDs idle - so the partition with
  // the shorter per-workgroup item count is taken, body groups on a tie (less feature traffic).
  int bg_lo, nper, n_streams, stream, vt_lo = 0, nvt = p.n_tiles;
  if ((gridDim.x & 7) == 0) {
    const int xcd = blockIdx.x & 7;
    n_streams = gridDim.x >> 3;
    stream = blockIdx.x >> 3;
    const int per_g = (p.nbg + 7) / 8, per_t = (p.n_tiles + 7) / 8;
    const int span_g = (per_g * p.n_tiles + n_streams - 1) / n_streams, span_t = (per_t * p.nbg + n_streams - 1) / n_streams;
    if (span_g <= span_t) {
      bg_lo = xcd * per_g;
      nper = max(0, min(per_g, p.nbg - bg_lo));
    } else {
      vt_lo = xcd * per_t;
      nvt = max(0, min(per_t, p.n_tiles - vt_lo));
      bg_lo = 0; nper = p.nbg;
    }
  } else {
    bg_lo = 0; nper = p.nbg;
    n_streams = gridDim.x;
    stream = blockIdx.x;
  }
  const int n_items = nvt * nper;
  // item order: blocks of bg_block body groups, vertex-tile-major inside a block - the features / joint transforms of
  // a block (1.4 MB per group) stay in the XCD's 4 MiB L2 while the bases stream through once per block
  const int PB = max(1, min(p.bg_block, max(nper, 1)));
  unsigned long long tacc[4] = {0, 0, 0, 0};
  (void)tacc;
  auto run_item = [&](int vti, int bg) {
    [[maybe_unused]] const unsigned long long item_t0 = LBS_NOW();
    const int vt = p.tiles ? p.tiles[vti] : vti;
    const int bt0 = bg * (4 * NB) + wave * NB;   // a body group of this kernel = 4 waves x NB tiles of 32 bodies
    __syncthreads();  // previous item: every wave is done with the metadata and with the stage ring
    const int j_lo = p.tj_off[vt];
    const int JT = p.tj_off[vt + 1] - j_lo;
    // (the thread index goes through an empty asm so that per-lane addresses derived from it are formed here, per item: as
    // invariants of the persistent loop they were kept alive across the whole item and spilled to scratch)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    for (int idx = tid * 4; idx < JT * 32; idx += 1024)
      *reinterpret_cast<f32x4*>(&w.s_W[idx]) = *reinterpret_cast<const f32x4*>(&p.tj_w[(size_t)j_lo * 32 + idx]);
    if (wave == 0) {
      if (lane < JT) w.s_jl[lane] = p.tj_idx[j_lo + lane];
      const int sl = (lane < 32) ? p.pick_slot[vt * 32 + lane] : -1;
      const int fl = (lane < 32) ? p.vflags[vt * 32 + lane] : 0;
      if (lane < 32) w.s_slot[lane] = sl;
      const unsigned long long mp = __ballot(sl >= 0), ms = __ballot((fl & 3) == 2);
      if (lane == 0) { w.s_masks[0] = (unsigned)mp; w.s_masks[1] = (unsigned)ms; }
    }
    f32x16 acc[3][NB];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int q = 0; q < NB; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][q][r] = 0.f;
    if (!(p.dbg & 2)) {
      if constexpr (NPL == 4) {      // NPL 4 = the mixed blend (mode 3)
        // the tiles that hold the PICKED vertices (markers, vertex joints, landmark corners: the 8 leading tiles of 328) keep the
        // two-plane split: what the environment reads as positions - and differentiates into directions (the eye landmarks are
        // centimetres apart and aim 7 m rays) - stays at the 1e-6 m level; the fp16 product only feeds the penetration COUNT
        if (vti < p.n_precise) {
          if constexpr (NBW == LBS_NB) lbs_blend_split<2>(p, acc, vt, bt0, lane, wave, sA, tacc);
          else lbs_blend_split2_small<NB>(p, acc, vt, bt0, lane, wave, sA);
        } else lbs_blend_mixed<NB>(p, acc, vt, bt0, lane, wave, sA, tacc);
      } else if constexpr (NBW == LBS_NB) lbs_blend_split<NPL>(p, acc, vt, bt0, lane, wave, sA, tacc);
    } else __syncthreads();  // the blend's barriers also publish the metadata
    if (p.dbg & 1) {
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < NB; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) sum += acc[c][q][r];
      if (sum == 123.456f) p.pene[0] = 1;
      return;
    }
    // mixed blend: the tiles that only feed the count (everything after the picked tiles) classify with the cheap product and
    // re-evaluate what it cannot decide
#ifdef EGX_LBS_NOFIX   // development builds: the cheap product decides alone (the round-5 kernel), for A/B timing
    constexpr bool FIX = false;
#else
    constexpr bool FIX = NPL == 4 && DO_SDF;
#endif
#ifdef EGX_LBS_VALU_SKIN   // development builds: the count-only tiles skinned on the VALU as well (fix-up only), for A/B timing
    lbs_epilogue<false, DO_SDF, LBS3_RB, lbs3_qcap<NB>(), NB, FIX, MS>(p, w, acc, vt, bt0, JT, FIX && vti >= p.n_precise);
#else
    // count-only tiles whose joint list fits one k-step (eight joints: 309 of the 328 tiles of the synthetic body) are skinned on
    // the matrix pipe; the tiles with picked vertices (exact positions) and the long lists take the VALU epilogue - the latter with
    // the fix-up band as well, since their blend product is the cheap one too.  The small wave tile (three workgroups per CU, 168
    // registers) has no room for the twelve operands: VALU epilogue throughout.
    if (FIX && NB == LBS_NB && vti >= p.n_precise && JT <= 8) lbs_epilogue_cell<LBS3_RB, lbs3_qcap<NB>(), NB, MS>(p, w, acc, vt, bt0, JT);
    else lbs_epilogue<false, DO_SDF, LBS3_RB, lbs3_qcap<NB>(), NB, FIX, MS>(p, w, acc, vt, bt0, JT, FIX && vti >= p.n_precise);
#endif
#ifdef EGX_LBS_TIMING
    w.et[4] += LBS_NOW() - item_t0; w.et[5] += 1;
#endif
  };
  // one loop for both item sources (the body is inlined once): a culled launch walks this XCD's list of active items
  // (egx_lbs_compact_kernel: an item whose 256 bodies are provably in free space for the whole vertex tile is not on it), dealt
  // round-robin to the XCD's workgroups; otherwise the blocked (tile, body group) order above
  const int* list = p.items ? p.items + (size_t)(blockIdx.x & 7) * p.items_stride : nullptr;
  const int i_lo = list ? (int)(blockIdx.x >> 3) : stream, i_step = list ? (int)(gridDim.x >> 3) : n_streams;
  const int i_hi = list ? p.item_counts[blockIdx.x & 7] : n_items;
  for (int item = i_lo; item < i_hi; item += i_step) {
    int vti, bg;
    if (list) {
      const int code = list[item];
      vti = code / p.nbg;
      bg = code - vti * p.nbg;
    } else {
      const int blk = item / (nvt * PB);
      const int pb = min(PB, nper - blk * PB);
      const int r = item - blk * nvt * PB;
      vti = vt_lo + r / pb;
      bg = bg_lo + blk * PB + r % pb;
    }
    run_item(vti, bg);
  }
#ifdef EGX_LBS_TIMING
  if (lane == 0) {
    for (int i = 0; i < 4; ++i) atomicAdd(&g_lbs_t[i], tacc[i]);
    atomicAdd(&g_lbs_t[9], w.et[0]); atomicAdd(&g_lbs_t[10], w.et[1]); atomicAdd(&g_lbs_t[11], w.et[2]); atomicAdd(&g_lbs_t[12], w.et[3]);
    atomicAdd(&g_lbs_t[13], w.et[4]); atomicAdd(&g_lbs_t[14], w.et[5]);
  }
#endif
}

// One table for both the instantiations whose dynamic-LDS cap is raised and the ones that can be launched: blend mode 1 | 2 | 3
// (NPL 3 | 2 | 4), with or without the SDF count, the small wave tile (mode 3 only), scene sets (with the count, large tile only).
int lbs_launch_fused3(const LbsParams& p, int mode, bool do_sdf, bool ms, int forced_tile, hipStream_t stream) {
  constexpr size_t lds3 = (size_t)LBS3_SHARED_BYTES + 4 * lbs3_wave_bytes<LBS_NB>();
  static const struct { void (*fn)(LbsParams); int mode; bool sdf, small, ms; } variants[] = {
      {egx_lbs_fused3_kernel<3, true>, 1, true, false, false},    {egx_lbs_fused3_kernel<3, false>, 1, false, false, false},
      {egx_lbs_fused3_kernel<2, true>, 2, true, false, false},    {egx_lbs_fused3_kernel<2, false>, 2, false, false, false},
      {egx_lbs_fused3_kernel<4, true>, 3, true, false, false},    {egx_lbs_fused3_kernel<4, false>, 3, false, false, false},
      {egx_lbs_fused3_kernel<4, true, 1>, 3, true, true, false},  {egx_lbs_fused3_kernel<4, false, 1>, 3, false, true, false},
      {egx_lbs_fused3_kernel<3, true, LBS_NB, true>, 1, true, false, true},
      {egx_lbs_fused3_kernel<2, true, LBS_NB, true>, 2, true, false, true},
      {egx_lbs_fused3_kernel<4, true, LBS_NB, true>, 3, true, false, true},
  };
  static LbsDeviceInfo devs[kMaxDevices];
  int num_cu = 0;
  auto raise_caps = [&]() -> int {
    for (const auto& v : variants)
      EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(v.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(v.small ? lbs3_lds_bytes<1>() : lds3)));
    return EGX_OK;
  };
  if (int rc = lbs_device_cus(devs, raise_caps, &num_cu)) return rc;
  const int n_items = p.nbg * p.n_tiles;
  // two persistent 4-wave workgroups per CU: one's VALU epilogue runs under the other's MFMA stages
  int wg_per_cu = 2;
#ifdef EGX_LBS_DEVELOPMENT
  if (const char* e = getenv("EGX_LBS_WG_PER_CU")) wg_per_cu = std::max(1, atoi(e));   // occupancy sensitivity (1 = one wave per SIMD)
#endif
  int grid3 = std::max(1, std::min(wg_per_cu * num_cu, n_items));
  if (grid3 >= 8) grid3 &= ~7;   // a multiple of 8: the kernel's XCD partition (body groups, or vertex tiles when groups are few)
  // mixed blend without culling, launches of at most 20 body groups of 256 (<= 256 agents x 20 frames): the small wave tile
  // (32 vertices x 32 bodies per wave, 128 bodies per workgroup item, three workgroups per CU) - finer items balance the
  // XCDs better and a third wave per SIMD helps where the launch is short: 640 bodies 0.086 -> 0.073 ms, 1 280 0.150 -> 0.116,
  // 2 560 0.250 -> 0.209, 5 120 0.461 -> 0.355; at 10 240 bodies the larger tile wins (0.686 against 0.734: the halved
  // item repeats the bases traffic and the barriers), profiles/r05_lbs_mixed.md section 5.  EGX_LBS_WAVE_TILE=1 | 2 forces one.
  const bool small_tile = forced_tile == 1 || (forced_tile != 2 && p.nbg <= 20);
  // set launches of two or more scenes always take the 32 x 64 tile: the small tile's epilogue has no registers for the body's
  // scene (its one-scene form already spills 5 VGPRs; a set form spilled 4), so it has no set instantiation
  const bool small = mode == 3 && small_tile && !p.items && !ms;
  LbsParams q = p;
  int grid = grid3;
  if (small) {
    q.nbg = egx_ceil_div(p.B, 128);
    q.bg_block = 2 * p.bg_block;
    const int n_items1 = q.nbg * q.n_tiles;
    int g1 = std::max(1, std::min(3 * num_cu, n_items1));
    if (g1 >= 8) g1 &= ~7;
    grid = g1;
  }
  for (const auto& v : variants)
    if (v.mode == mode && v.sdf == do_sdf && v.small == small && v.ms == ms) {
      hipLaunchKernelGGL(v.fn, dim3(grid), dim3(256), small ? lbs3_lds_bytes<1>() : lds3, stream, q);
      return EGX_OK;
    }
  egx_set_error("no split-blend LBS kernel for this call");
  return EGX_ERR_ARG;
}

#ifdef EGX_LBS_TIMING
extern "C" int egx_lbs_timing_read(unsigned long long* out16, int reset) {
  EGX_HIP_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_lbs_t), 16 * sizeof(unsigned long long)));
  if (reset) {
    unsigned long long z[16] = {0};
    EGX_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_lbs_t), z, sizeof(z)));
  }
  return EGX_OK;
}
#endif
