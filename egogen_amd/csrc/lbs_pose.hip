// LBS forward, first launch: per-body pose features, rigid chain and joint transforms (and, for the mixed blend, the body's position
// error bound and the operands of the matrix-pipe skinning).
#include "lbs.h"

// ------------------------------------------------------------------------------------------------
// kernel 1: per-body pose features, rigid chain, joint transforms
// ------------------------------------------------------------------------------------------------
// MS (scene sets, egx_lbs_forward_scenes): the agent's scene - agent_scene[agent] of the set's table `scenes` - replaces `sdf` in the
// canonical-frame -> SDF-cell map, and a body whose agent names no scene of the set gets the count -1 instead of 0.
template <bool MS>
__global__ __launch_bounds__(256) void egx_pose_chain_kernel(const PoseConsts* __restrict__ pc,
                                                             const float* __restrict__ xb,
                                                             const float* __restrict__ betas, int B, int fpa,
                                                             float* __restrict__ feat,   // packed B operand (fp32 blend) or null
                                                             unsigned short* __restrict__ feat3,  // bf16x3 planes or null
                                                             f32x4* __restrict__ A4,     // [bt][55][3][32]
                                                             float* __restrict__ out_joints, int joints_ld,
                                                             float template_lo_feat /* 1 in the two-plane blend mode */,
                                                             unsigned short* __restrict__ feat4 /* mixed-blend image (mode 3) or null */,
                                                             int* __restrict__ zero_counts /* [B] cleared here, or null */,
                                                             const int* __restrict__ agent_of_slot /* culled launches: slot order */,
                                                             float* __restrict__ fvec /* [64][Bp] |beta|, ||R_j - I||_F or null */,
                                                             float* __restrict__ jpos /* [55][3][Bp] posed joints + transl or null */,
                                                             int Bp,
                                                             float* __restrict__ fix_e /* [Bp] per slot: position error bound of the mixed blend (metres) or null */,
                                                             int* __restrict__ fix_stats /* [1] cleared here, or null */,
                                                             unsigned short* __restrict__ skinB /* matrix-pipe skinning operands (see SKIN_BT_BYTES) or null */,
                                                             f32x4* __restrict__ cinit /* [Bp] per slot: cell coordinates of the body's translation */,
                                                             const float* __restrict__ R0, const float* __restrict__ T0, SdfDev sdf,
                                                             const SdfSceneDev* __restrict__ scenes, const int* __restrict__ agent_scene,
                                                             int n_scenes) {
  __shared__ float sJ[4][NJ][3];
  __shared__ float sG[4][NJ][12];
  __shared__ __attribute__((aligned(16))) unsigned short sF3[4][3][KS3 * 16];  // bf16x3 planes of the 4 bodies of the block
  __shared__ __attribute__((aligned(16))) unsigned short sF4[4][KS3 * 16];     // fp16 values (mixed blend, k-steps 1..28)
  const int w = threadIdx.x >> 6, j = threadIdx.x & 63;
  // a block works on four SLOTS of the operand buffers; slot s holds body agent_of_slot[s / fpa] * fpa + s % fpa (identity
  // without the table): inputs and per-body outputs are addressed by body, the GEMM operands by slot
  const int slot = blockIdx.x * 4 + w;
  const bool live = slot < B;
  const int ss = live ? slot : B - 1;
  const int b = agent_of_slot ? agent_of_slot[ss / fpa] * fpa + ss % fpa : ss;
  [[maybe_unused]] int scn = 0;   // MS: the agent's scene, -1 when agent_scene names none of the set (reads below use scene 0)
  if constexpr (MS) {
    const int v = agent_scene[b / fpa];
    scn = (v >= 0 && v < n_scenes) ? v : -1;
  }
  if (zero_counts && live && j == 0) zero_counts[b] = scn < 0 ? -1 : 0;   // the SDF epilogue of the skinning kernel adds to these
  if (fix_stats && blockIdx.x == 0 && threadIdx.x <= LBS_FIX_NQ) fix_stats[threadIdx.x == 0 ? 0 : LBS_FIX_CNT0 + 32 * (threadIdx.x - 1)] = 0;
  const int bb = b;
  const float* x = xb + (size_t)bb * EGX_XB_DIM;
  const float* be = betas + (size_t)(bb / fpa) * 10;
  const int bt = ss >> 5, n = ss & 31;
  float* featb = feat ? feat + (size_t)bt * KGROUPS * 64 * 4 : nullptr;  // tile base
  unsigned short* feat3b = feat3 ? feat3 + (size_t)bt * KS3 * 3 * 64 * 8 : nullptr;
  auto feat_store = [&](int k, float v) {
    if (featb && k < KDIM) {
      const int s = k >> 1, kk = k & 1;
      featb[((s >> 2) * 64 + (kk * 32 + n)) * 4 + (s & 3)] = v;
    }
    if (feat3b) {  // staged in LDS; written out below as whole 16-byte operand fragments
      unsigned short h[3];
      egx_bf16_split3(v, h);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) sF3[w][pl][k] = h[pl];
      if (feat4) sF4[w][k] = egx_f16_rne(v);   // the mixed blend reads k-steps 1..28 as one fp16 plane
    }
  };
  float R[9], Jr[3];
  if (j < NJ) {
    {
    // (lbs_joint_rotation, spelled out: through the shared function the compiler contracts these products differently - last-bit
    // changes of R that the egosensing rays, aimed by eye landmarks centimetres apart, amplify past the parity floor)
    float a[3] = {0.f, 0.f, 0.f};
    if (j == 0) {
      a[0] = x[3]; a[1] = x[4]; a[2] = x[5];
    } else if (j <= 21) {
      a[0] = x[6 + 3 * (j - 1)]; a[1] = x[7 + 3 * (j - 1)]; a[2] = x[8 + 3 * (j - 1)];
    } else if (j >= 25) {
      const int side = (j >= 40) ? 1 : 0;
      const int o = 3 * (j - (side ? 40 : 25));
      const float* comps = pc->hand_comps + side * 12 * 45;
      const float* pca = x + 69 + side * 12;
      for (int c = 0; c < 3; ++c) {
        float s = 0.f;
        for (int k = 0; k < 12; ++k) s += pca[k] * comps[k * 45 + o + c];
        a[c] = s + pc->hand_mean[side * 45 + o + c];
      }
    }
    const float ex = a[0] + 1e-8f, ey = a[1] + 1e-8f, ez = a[2] + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float rx = a[0] / angle, ry = a[1] / angle, rz = a[2] / angle;
    const float sn = sinf(angle), cs = 1.f - cosf(angle);
    R[0] = 1.f + cs * (-(ry * ry + rz * rz)); R[1] = -sn * rz + cs * (rx * ry);     R[2] = sn * ry + cs * (rx * rz);
    R[3] = sn * rz + cs * (rx * ry);          R[4] = 1.f + cs * (-(rx * rx + rz * rz)); R[5] = -sn * rx + cs * (ry * rz);
    R[6] = -sn * ry + cs * (rx * rz);         R[7] = sn * rx + cs * (ry * rz);      R[8] = 1.f + cs * (-(rx * rx + ry * ry));
    }
    for (int c = 0; c < 3; ++c) {
      float s = pc->J_template[j * 3 + c];
      for (int k = 0; k < 10; ++k) s += be[k] * pc->J_shapedirs[(j * 3 + c) * 10 + k];
      Jr[c] = s;
      sJ[w][j][c] = s;
    }
  }
  float fix_vb = 0.f;   // the body's bound of |v_posed| (mixed blend: see LBS_FIX_SLACK_M)
  if (fix_e) {   // wave-uniform: every lane of the body's wave takes part in the reductions
    // lane j: joint j's nine features (k = k0 + e; the fp16 k-steps hold k = 16..463), lanes 0..9: the shape term
    float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // |dF_H|^2, |f~_H|^2, |F|^2, L1 form, two-plane pose, sum |F_j|_1 C_j, shape
    if (j >= 1 && j < NJ && (j < 22 || j > 24)) {
      const int k0 = 10 + egx_compact_joint(j) * 9;
      float adf = 0.f, aft = 0.f, af = 0.f, afb = 0.f;
      for (int e = 0; e < 9; ++e) {
        const float dlt = R[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
        s[2] += dlt * dlt;
        af += fabsf(dlt);
        if (k0 + e >= 16 && k0 + e < 464) {
          const float h = (float)(_Float16)dlt;   // what the fp16 plane of the feature image holds (egx_f16_rne)
          const float d = h - dlt;                // exact
          s[0] += d * d; s[1] += h * h;
          adf += fabsf(d); aft += fabsf(h);
        } else {
          afb += fabsf(dlt);
        }
      }
      s[3] = adf * pc->fix_c[j] + aft * pc->fix_d[j];
      s[4] = afb * pc->fix_c[j];
      s[5] = af * pc->fix_c[j];
    }
    if (j < 10) s[6] = fabsf(be[j]) * pc->shape_c[j];
#pragma unroll
    for (int i = 0; i < 7; ++i)
      for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o);
    const float prod = fminf(sqrtf(s[0]) * pc->fix_pf + sqrtf(s[1]) * pc->fix_dpf, s[3]) + LBS_TWO_PLANE_ERR * (s[4] + s[6]);
    const float offs = (s[6] + fminf(sqrtf(s[2]) * pc->fix_pf, s[5])) * LBS_FIX_MARGIN;
    fix_vb = pc->vt_max + offs;
    const float accr = 5.9604645e-8f * (LBS_ACC_ADDS_OFFSETS * offs + LBS_ACC_ADDS_LAST * fix_vb);
    if (live && j == 0) fix_e[slot] = pc->w_abs_max * (prod + accr) * LBS_FIX_MARGIN + LBS_FIX_SLACK_M;
  }
  if (j < NJ) {
    if (live && fvec) {
      if (j < 10) fvec[(size_t)j * Bp + slot] = fabsf(be[j]);
      if (j >= 1 && (j < 22 || j > 24)) {
        float q = 0.f;
        for (int e = 0; e < 9; ++e) {
          const float dlt = R[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
          q += dlt * dlt;
        }
        fvec[(size_t)(10 + egx_compact_joint(j)) * Bp + slot] = sqrtf(q) * 1.000001f;
      }
    }
    if (live) {
      if (j < 10) feat_store(j, be[j]);
      if (j >= 1 && (j < 22 || j > 24)) {
        const int k0 = 10 + egx_compact_joint(j) * 9;
        for (int e = 0; e < 9; ++e) feat_store(k0 + e, R[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f));
      }
      // column 469 multiplies the template column of the bases (acc = v_template + offsets); column 470 multiplies the
      // third bf16 term of the template (bf16x3 bases only): switched on in the two-plane blend mode, where the product keeps
      // 16 bits per operand - enough for the centimetre-scale offsets, not for the metre-scale template; 471 is padding
      if (j >= 22 && j <= 24) feat_store(KACT + (j - 22), j == 22 ? 1.f : (j == 23 ? template_lo_feat : 0.f));
      if (feat3b && j >= 22 && j <= 24) {  // bf16x3 pads K to 480: columns 472..479
        for (int k = KDIM + (j - 22); k < KS3 * 16; k += 3) feat_store(k, 0.f);
      }
    }
  }
  __syncthreads();
  if (feat3) {
    // k = 16 s + 8 half + e  ->  [bt][s][plane][half*32 + n][e]: one 16-byte fragment per (s, plane, half, body); the four
    // bodies of the block are neighbours in n, so a quarter-wave writes 64 contiguous bytes
    for (int c = threadIdx.x; c < KS3 * 3 * 2 * 4; c += 256) {
      const int wb = c & 3, hf = (c >> 2) & 1, pl = (c >> 3) % 3, sidx = c / 24;
      const int body = blockIdx.x * 4 + wb;   // slot
      if (body < B) {
        const int4 frag = *reinterpret_cast<const int4*>(&sF3[wb][pl][sidx * 16 + hf * 8]);
        unsigned short* dst = feat3 + ((((size_t)(body >> 5) * KS3 + sidx) * 3 + pl) * 64 + hf * 32 + (body & 31)) * 8;
        *reinterpret_cast<int4*>(dst) = frag;
      }
    }
  }
  if (feat3 && feat4) {
    // the mixed image: 32 pieces per body tile (two bf16 planes of k-steps 0 and 29, one fp16 plane of k-steps 1..28)
    for (int c = threadIdx.x; c < M4_FEAT_PIECES * 2 * 4; c += 256) {
      const int wb = c & 3, hf = (c >> 2) & 1, piece = c >> 3;
      const int sidx = piece < 2 ? 0 : (piece < 30 ? piece - 1 : 29), pl = piece < 2 ? piece : (piece < 30 ? 0 : piece - 30);
      const int body = blockIdx.x * 4 + wb;   // slot
      if (body < B) {
        const unsigned short* src = (piece >= 2 && piece < 30) ? &sF4[wb][sidx * 16 + hf * 8] : &sF3[wb][pl][sidx * 16 + hf * 8];
        const int4 frag = *reinterpret_cast<const int4*>(src);
        unsigned short* dst = feat4 + (((size_t)(body >> 5) * M4_FEAT_PIECES + piece) * 64 + hf * 32 + (body & 31)) * 8;
        *reinterpret_cast<int4*>(dst) = frag;
      }
    }
  }

  const int par = (j < NJ) ? pc->parents[j] : -1;
  const int dep = (j < NJ) ? pc->depth[j] : -1;
  float rel[3] = {0.f, 0.f, 0.f};
  if (j < NJ) {
    for (int c = 0; c < 3; ++c) rel[c] = Jr[c] - (par >= 0 ? sJ[w][par][c] : 0.f);
  }
  float G[12];
  const int max_depth = pc->max_depth;
  for (int d = 0; d <= max_depth; ++d) {
    if (dep == d) {
      if (par < 0) {
        for (int r = 0; r < 3; ++r) {
          G[r * 4 + 0] = R[r * 3 + 0]; G[r * 4 + 1] = R[r * 3 + 1]; G[r * 4 + 2] = R[r * 3 + 2]; G[r * 4 + 3] = rel[r];
        }
      } else {
        const float* P = sG[w][par];
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c)
            G[r * 4 + c] = P[r * 4 + 0] * R[0 * 3 + c] + P[r * 4 + 1] * R[1 * 3 + c] + P[r * 4 + 2] * R[2 * 3 + c];
          G[r * 4 + 3] = P[r * 4 + 0] * rel[0] + P[r * 4 + 1] * rel[1] + P[r * 4 + 2] * rel[2] + P[r * 4 + 3];
        }
      }
      for (int e = 0; e < 12; ++e) sG[w][j][e] = G[e];
    }
    // sG[w] is private to this wave (one body per wave) and a wave's LDS operations complete in order: the next level's reads
    // only have to stay behind these writes in program order - no workgroup barrier per level of the tree
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (skinB) {   // block-uniform
    // A'_j = Mc A_j: the joint transform followed by the agent's canonical frame -> SDF-cell map (the folded affine map of the
    // fused kernel's epilogue scaled by 1/4, egx_sdf_coarse_at_cell); the constant part Mc transl + tc stays in fp32 (cinit)
    const int ag = bb / fpa;
    float Mc[9], tcv[3];
    {
      if constexpr (MS) sdf = egx_sdf_scene(sdf, scenes[max(scn, 0)]);
      const float kk[3] = {sdf.scale * (float)sdf.d0 * 0.5f, sdf.scale * (float)sdf.d1 * 0.5f, sdf.scale * (float)sdf.d2 * 0.5f};
      const float cc[3] = {sdf.cx, sdf.cy, sdf.cz};
      const float dd[3] = {(float)sdf.d0, (float)sdf.d1, (float)sdf.d2};
      for (int a = 0; a < 3; ++a) {
        for (int e = 0; e < 3; ++e) Mc[a * 3 + e] = 0.25f * (kk[a] * (R0 ? R0[(size_t)ag * 9 + a * 3 + e] : ((a == e) ? 1.f : 0.f)));
        const float tw = kk[a] * ((T0 ? T0[(size_t)ag * 3 + a] : 0.f) - cc[a]) + (dd[a] - 1.f) * 0.5f;
        tcv[a] = fmaf(0.25f, tw, 1.f);
      }
    }
    float tn = 0.f;
    if (j < NJ) {
      float Arow[3][4];
      for (int r = 0; r < 3; ++r) {
        Arow[r][0] = G[r * 4 + 0]; Arow[r][1] = G[r * 4 + 1]; Arow[r][2] = G[r * 4 + 2];
        Arow[r][3] = G[r * 4 + 3] - (G[r * 4 + 0] * Jr[0] + G[r * 4 + 1] * Jr[1] + G[r * 4 + 2] * Jr[2]);
      }
      tn = sqrtf(Arow[0][3] * Arow[0][3] + Arow[1][3] * Arow[1][3] + Arow[2][3] * Arow[2][3]);
      // the joint's two records (hi and mid plane: 12 entries each), packed in registers and stored straight to the image:
      // 16 + 8 bytes per plane at [joint][plane][n] (the four bodies of the block are neighbours in n: 64-byte runs)
      unsigned pk[2][6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        unsigned short hh[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int a = (2 * i + u) >> 2, c = (2 * i + u) & 3;
          egx_bf16_split3(Mc[a * 3 + 0] * Arow[0][c] + Mc[a * 3 + 1] * Arow[1][c] + Mc[a * 3 + 2] * Arow[2][c], hh[u]);
        }
        pk[0][i] = (unsigned)hh[0][0] | ((unsigned)hh[1][0] << 16);
        pk[1][i] = (unsigned)hh[0][1] | ((unsigned)hh[1][1] << 16);
      }
      if (live) {
        unsigned short* base = skinB + (size_t)bt * (SKIN_BT_BYTES / 2);
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
          const size_t rec = ((size_t)j * 2 + pl) * 32 + n;
          *reinterpret_cast<uint4*>(base + rec * 8) = make_uint4(pk[pl][0], pk[pl][1], pk[pl][2], pk[pl][3]);
          *reinterpret_cast<uint2*>(base + (size_t)SKIN_BT_A * 8 + rec * 4) = make_uint2(pk[pl][4], pk[pl][5]);
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) tn = fmaxf(tn, __shfl_xor(tn, o));
    if (live && j == 0) {
      f32x4 ci;
      for (int a = 0; a < 3; ++a) ci[a] = fmaf(Mc[a * 3 + 0], x[0], fmaf(Mc[a * 3 + 1], x[1], fmaf(Mc[a * 3 + 2], x[2], tcv[a])));
      ci[3] = 0.f;
      cinit[slot] = ci;
      // the two-plane products of the skinning add to the body's position error bound (see LBS_SKIN_ERR)
      if (fix_e) fix_e[slot] += LBS_SKIN_ERR * pc->w_abs_max * (fix_vb + tn) * LBS_FIX_MARGIN;
    }
  }
  if (j < NJ && live) {
    // relative transform: translation column minus R_g * rest joint (smplx batch_rigid_transform)
    for (int r = 0; r < 3; ++r) {
      const float t = G[r * 4 + 3] - (G[r * 4 + 0] * Jr[0] + G[r * 4 + 1] * Jr[1] + G[r * 4 + 2] * Jr[2]);
      f32x4 row = {G[r * 4 + 0], G[r * 4 + 1], G[r * 4 + 2], t};
      A4[(((size_t)bt * NJ + j) * 3 + r) * 32 + n] = row;
    }
    if (out_joints) {
      float* o = out_joints + ((size_t)b * joints_ld + j) * 3;
      o[0] = G[3] + x[0]; o[1] = G[7] + x[1]; o[2] = G[11] + x[2];
    }
    if (jpos) {
      jpos[(size_t)(j * 3 + 0) * Bp + slot] = G[3] + x[0];
      jpos[(size_t)(j * 3 + 1) * Bp + slot] = G[7] + x[1];
      jpos[(size_t)(j * 3 + 2) * Bp + slot] = G[11] + x[2];
    }
  }
}

void lbs_launch_pose(bool ms, hipStream_t stream, const LbsPoseArgs& a) {
  hipLaunchKernelGGL(ms ? egx_pose_chain_kernel<true> : egx_pose_chain_kernel<false>, dim3(egx_ceil_div(a.B, 4)), dim3(256), 0, stream, a.pc, a.xb,
                     a.betas, a.B, a.fpa, a.feat, a.feat3, a.A4, a.out_joints, a.joints_ld, a.template_lo_feat, a.feat4, a.zero_counts,
                     a.agent_of_slot, a.fvec, a.jpos, a.Bp, a.fix_e, a.fix_stats, a.skinB, a.cinit, a.R0, a.T0, a.sdf, a.scenes, a.agent_scene,
                     a.n_scenes);
}
