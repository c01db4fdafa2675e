// The squared-distance tile of sv_knn_classify (include/splitvae.h: norm, distance) as a header: knn_norm_kernel's body and
// knn_tile_kernel's staging, K loop and distance epilogue of knn.hip, statement for statement, for the kernels that need the same bits
// (tsne.hip).  knn.hip keeps its own copy: calling this header from knn_tile_kernel changed that kernel's register allocation (585 lines
// of its assembly), and no existing kernel's code changes here.  tests/test_gpu_tsne.py holds the two to the same bits.
//   dist_norm_rows   n(v) = sum_j v_j^2 per row: one wave per row, lanes stride j, then the 64-lane butterfly -- one order per row
//   dist_tile_64x64  a workgroup of 256 threads: the 64 rows m0 .. of q against the 64 rows n0 .. of r (rows >= Nq / >= c1 read as zero):
//                    the dense_f32.hip K loop (v_mfma_f32_16x16x4_f32 over the whole of L, zero-padded to 32, k = 4 kk + lane / 16
//                    ascending), then d = max(0, (n(q) + n(r)) - 2 dot) into the LDS tile sD [64][DP].  Ends behind a barrier: every
//                    thread may read all of sD.  Begins with a barrier of its own behind the first staging, so a caller's reads of the
//                    previous tile's sD are over before this one writes.
// LDS: operands as [k][m] images with rows of 80 floats (320 B: 16-B aligned; the ds_read_b32 bank is dword % 32 per 32-lane half,
// a half reads k rows 2 apart in lk = 0 / 1, 80 % 32 = 16: conflict-free; the staging writes put 32 consecutive m of one k row
// into a half: conflict-free); the distance tile as [m][68] (the accumulator rows lk 4 apart land 16 banks apart).
#pragma once
#include "eval_common.hip.h"

constexpr int DT_BM = 64, DT_BN = 64, DT_BK = 32, DT_LP = 80, DT_DP = 68;

__device__ __forceinline__ void dist_norm_rows(const float* __restrict__ v, int ld, int N, int L, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;                            // whole waves leave
  const float* __restrict__ p = v + row * ld;
  float s = 0.f;
  for (int j = lane; j < L; j += 64) s += p[j] * p[j];
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

// rows mn0 + (tid & 63), k piece k0 + (tid >> 6) * 8: 8 floats of one row (k contiguous)
__device__ __forceinline__ void dist_load(const float* __restrict__ P, int ld, int mn0, int k0, int MN, int L, int tid, bool vec, float (&r)[8]) {
  const int row = mn0 + (tid & 63), k = k0 + (tid >> 6) * 8;
  const bool any = row < MN;
  const int lim = L - k;
  const float* p = P + (int64_t)row * ld + k;
  if (any && vec && lim >= 8) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (any && i < lim) ? p[i] : 0.f;
  }
}
__device__ __forceinline__ void dist_store(float* s, int tid, const float (&r)[8]) {
  const int m = tid & 63, k = (tid >> 6) * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[(k + i) * DT_LP + m] = r[i];
}

// nqv: the norms of this lane's accumulator rows m0 + wm + i * 16 + lk * 4 + r (0 past Nq); nr: the norms of r
__device__ __forceinline__ void dist_tile_64x64(const float* __restrict__ q, int ldq, int m0, int Nq, bool vecq, const float* __restrict__ r, int ldr,
                                                int n0, int c1, bool vecr, int L, const float (&nqv)[2][4], const float* __restrict__ nr,
                                                float (*sA)[DT_BK * DT_LP], float (*sB)[DT_BK * DT_LP], float* sD) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nks = (L + DT_BK - 1) / DT_BK;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, lr = lane & 15, lk = lane >> 4;
  float ra[8], rb[8];
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  dist_load(q, ldq, m0, 0, Nq, L, tid, vecq, ra);
  dist_load(r, ldr, n0, 0, c1, L, tid, vecr, rb);
  dist_store(sA[0], tid, ra);
  dist_store(sB[0], tid, rb);
  __syncthreads();                               // (also: every wave is done with the previous tile's sD)
  for (int ks = 0; ks < nks; ++ks) {
    const int buf = ks & 1;
    const bool more = ks + 1 < nks;
    if (more) {
      dist_load(q, ldq, m0, (ks + 1) * DT_BK, Nq, L, tid, vecq, ra);
      dist_load(r, ldr, n0, (ks + 1) * DT_BK, c1, L, tid, vecr, rb);
    }
    const float* cA = sA[buf];
    const float* cB = sB[buf];
#pragma unroll
    for (int kk = 0; kk < DT_BK / 4; ++kk) {
      const int k = kk * 4 + lk;
      const float a0 = cA[k * DT_LP + wm + lr], a1 = cA[k * DT_LP + wm + 16 + lr];
      const float b0 = cB[k * DT_LP + wn + lr], b1 = cB[k * DT_LP + wn + 16 + lr];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (more) {
      dist_store(sA[buf ^ 1], tid, ra);
      dist_store(sB[buf ^ 1], tid, rb);
    }
    __syncthreads();
  }
  // D: row = (lane >> 4) * 4 + reg, column = lane & 15 of each fragment.  d = max(0, (n(q) + n(r)) - 2 dot)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int nl = wn + j * 16 + lr;
    const float nrv = n0 + nl < c1 ? nr[n0 + nl] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int ml = wm + i * 16 + lk * 4 + rr;
        sD[ml * DT_DP + nl] = fmaxf(0.f, (nqv[i][rr] + nrv) - 2.f * acc[i][j][rr]);
      }
  }
  __syncthreads();
}
