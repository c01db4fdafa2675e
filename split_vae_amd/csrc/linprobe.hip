// Linear label probe of the latents: softmax regression on frozen rows by Boehning's fixed-Hessian majorise-minimise step.
// The definition (logits, softmax, residual, loss, the folds, the step, the trajectory index) is pinned in include/splitvae.h
// (sv_linprobe_*); this file is the kernels.
//   lp_tile_kernel<NJ>  workgroup = 64 rows of x against the C classes (NJ = the 16-column fragments that hold one): knn_tile_kernel's
//                       K loop (v_mfma_f32_16x16x4_f32 over the whole of L, k = 4 kk + lane / 16 ascending), W rounded to fp32 while
//                       it is staged beside the x tile.  The logits go through LDS to one thread per row: max, expf, the sum over the
//                       classes in ascending order, the residual row and the row's loss.  Fit: the 64 x Cp residual tile is written
//                       as whole rows (Cp = C padded to 16, the pad columns 0) and the tile's loss (rows ascending, fp64).  Predict:
//                       the argmax, the hits (integer atomics) and the same loss partial.
//   lp_atb_kernel       A^T (rows x cols) per chunk of 256 rows, A = [x 1]: a wave owns 16 features and up to 64 columns, walks the
//                       chunk's rows four at a time in ascending order (the MFMA's k) and leaves its fp32 accumulators as the chunk's
//                       partial.  Operands come straight from global memory: a 16-lane group reads 64 contiguous bytes of a row.
//                       cols = the residual (the gradient) or A itself (the Gram matrix: fragments below the diagonal are skipped).
//   lp_fold_kernel      one thread per element: the chunk partials in chunk order, fp64.  Gram: S (the lower triangle mirrored from
//                       the upper).  Fit: G = sum / N + l2 W; one further workgroup folds the tiles' losses and the penalty -> loss_t
//   lp_step_kernel      workgroup 0: gmax_t = max |G|, the trajectory index moves on; every workgroup: 4 rows of W <- W - P G (fp64, j ascending,
//                       P's rows and G through LDS in slices of 64)
//   lp_state_kernel     the trajectory index of a call: 0, or (resume) one back: the last pass is made again and gives the same bits
//   lp_mean_kernel      predict: the tiles' losses -> loss[0]
// A fit iteration is four launches and reads x twice (logits, gradient); the residual goes through memory (N x Cp fp32).
#include "eval_common.hip.h"

namespace {

constexpr int BM = 64, BK = 16, LPA = 80, LPB = 80, LPZ = 65;
constexpr int LP_CHUNK = 256;                      // rows per fp32 partial of A^T (.) (sv_linprobe_chunk_rows)

struct LpTileArgs {
  const float* x; const uint8_t* cls; const double* w;
  float* r; double* part_loss; int32_t* pred; unsigned long long* acc;
  int ldx, N, L, C, Cp, vecx, predict;
};

template <int NJ> __global__ __launch_bounds__(256) void lp_tile_kernel(const LpTileArgs g) {
  __shared__ __attribute__((aligned(16))) float sA[2][BK * LPA];
  __shared__ __attribute__((aligned(16))) float sB[2][BK * LPB];
  __shared__ float sZ[BM * LPZ];
  __shared__ float sL[BM];
  __shared__ int sHit;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int m0 = blockIdx.x * BM;
  const int nks = (g.L + BK - 1) / BK;
  const int wm = wave * 16;
  // staging roles: x -- row tid & 63, 4 floats at k = (tid >> 6) * 4; W -- k row tid >> 4, the 4 classes (tid & 15) * 4 ..
  const int arow = m0 + (tid & 63), ak = (tid >> 6) * 4;
  const float* ap = g.x + (int64_t)arow * g.ldx + ak;
  const bool aok = arow < g.N;
  const int bk = tid >> 4, bc = (tid & 15) * 4;
  float ra[4], rb[4];
  auto load = [&](int k0) {
    const int la = g.L - (k0 + ak);
    if (aok && g.vecx && la >= 4) {
      const float4 v = *(const float4*)(ap + k0);
      ra[0] = v.x; ra[1] = v.y; ra[2] = v.z; ra[3] = v.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) ra[i] = (aok && i < la) ? ap[k0 + i] : 0.f;
    }
    const int l = k0 + bk;
#pragma unroll
    for (int i = 0; i < 4; ++i) rb[i] = (l < g.L && bc + i < g.C) ? (float)g.w[(int64_t)l * g.C + bc + i] : 0.f;
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sA[buf][(ak + i) * LPA + (tid & 63)] = ra[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) sB[buf][bk * LPB + bc + i] = rb[i];
  };
  f32x4 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (tid == 0) sHit = 0;
  load(0);
  store(0);
  __syncthreads();
  for (int ks = 0; ks < nks; ++ks) {
    const int buf = ks & 1;
    const bool more = ks + 1 < nks;
    if (more) load((ks + 1) * BK);
    const float* cA = sA[buf];
    const float* cB = sB[buf];
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      const int k = kk * 4 + lk;
      const float a = cA[k * LPA + wm + lr];
      float b[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) b[j] = cB[k * LPB + j * 16 + lr];
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[j], acc[j], 0, 0, 0);
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }
  // D: row = (lane >> 4) * 4 + reg, column = lane & 15 of each fragment.  z = dot + bias
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = j * 16 + lr;
    const float bias = c < g.C ? (float)g.w[(int64_t)g.L * g.C + c] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) sZ[(wm + lk * 4 + r) * LPZ + c] = acc[j][r] + bias;
  }
  __syncthreads();
  const int rows = min(BM, g.N - m0);
  if (tid < rows) {
    float* z = sZ + tid * LPZ;
    const int row = m0 + tid;
    const int y = g.cls ? (int)g.cls[row] : g.C;
    const bool valid = y < g.C;
    float m = z[0];
    int best = 0;
    for (int c = 1; c < g.C; ++c) {
      if (z[c] > z[best]) best = c;                // the first maximum: ties to the lower class
      m = fmaxf(m, z[c]);
    }
    const float zy = valid ? z[y] : m;
    float s = 0.f;
    for (int c = 0; c < g.C; ++c) {                // ascending c
      const float e = expf(z[c] - m);
      z[c] = e;
      s += e;
    }
    sL[tid] = valid ? logf(s) - (zy - m) : 0.f;
    if (g.predict) {
      g.pred[row] = best;
      if (valid && best == y) atomicAdd(&sHit, 1); // integer: any order, same sum
    } else {
      for (int c = 0; c < g.C; ++c) {
        const float p = z[c] / s;
        z[c] = valid ? p - (c == y ? 1.f : 0.f) : 0.f;
      }
    }
  }
  __syncthreads();
  if (!g.predict) {
    for (int e = tid; e < rows * g.Cp; e += 256) {
      const int rr = e / g.Cp, c = e - rr * g.Cp;
      g.r[(int64_t)(m0 + rr) * g.Cp + c] = c < g.C ? sZ[rr * LPZ + c] : 0.f;
    }
  }
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < rows; ++i) s += (double)sL[i];       // rows in ascending order
    g.part_loss[blockIdx.x] = s;
    if (g.predict && g.acc) {
      if (sHit) atomicAdd(&g.acc[0], (unsigned long long)sHit);
      if (blockIdx.x == 0) atomicAdd(&g.acc[1], (unsigned long long)g.N);
    }
  }
}

// part[chunk][f][c] (fp32, pitch cpitch) = sum over the chunk's rows, ascending, of A[row][f] * M[row][c]; A = [x 1].
// m = NULL: M = A (the Gram matrix), the fragments with every column below the wave's features are skipped.
__global__ __launch_bounds__(256) void lp_atb_kernel(const float* __restrict__ x, int ldx, int N, int L, const float* __restrict__ m, int ldm,
                                                     int ncols, int cpitch, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int F = L + 1, nff = (F + 15) >> 4, ncf = cpitch >> 4;
  const int fi = blockIdx.y * 4 + wave;
  if (fi >= nff) return;                           // whole waves leave; the kernel has no barrier
  const int chunk = blockIdx.x, r0 = chunk * LP_CHUNK;
  const int steps = (min(LP_CHUNK, N - r0) + 3) >> 2;
  const int f = fi * 16 + lr;
  const bool fx = f < L;
  const float fconst = f == L ? 1.f : 0.f;
  const float* __restrict__ xa = x + (fx ? f : 0);
  bool jok[4], cx[4];
  float cconst[4];
  const float* cp[4];
  int64_t cld;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cj = blockIdx.z * 4 + j, c = cj * 16 + lr;
    jok[j] = cj < ncf && (m != nullptr || cj >= fi);
    if (m) { cx[j] = c < ncols; cconst[j] = 0.f; cp[j] = m + (cx[j] ? c : 0); }
    else { cx[j] = c < L; cconst[j] = c == L ? 1.f : 0.f; cp[j] = x + (cx[j] ? c : 0); }
  }
  if (!(jok[0] || jok[1] || jok[2] || jok[3])) return;       // a wave of the Gram pass wholly below the diagonal
  cld = m ? ldm : ldx;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int kk = 0; kk < steps; ++kk) {
    const int row = r0 + kk * 4 + lk;
    const bool rok = row < N;                      // a row past N is a zero, whatever the memory behind it holds
    const float a = rok ? (fx ? xa[(int64_t)row * ldx] : fconst) : 0.f;
    float b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = (rok && jok[j]) ? (cx[j] ? cp[j][(int64_t)row * cld] : cconst[j]) : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (jok[j]) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[j], acc[j], 0, 0, 0);   // jok is wave-uniform
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!jok[j]) continue;
    const int c = (blockIdx.z * 4 + j) * 16 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ff = fi * 16 + lk * 4 + r;
      if (ff < F) part[((int64_t)chunk * F + ff) * cpitch + c] = acc[j][r];
    }
  }
}

__device__ __forceinline__ double lp_fold(const float* __restrict__ p, int64_t stride, int nchunks) {
  double sum = 0.0;
  int ch = 0;
  for (; ch + 8 <= nchunks; ch += 8) {             // eight loads in flight, added in chunk order
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = p[(ch + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += (double)t[u];
  }
  for (; ch < nchunks; ++ch) sum += (double)p[ch * stride];
  return sum;
}

__global__ __launch_bounds__(256) void lp_gram_fold_kernel(const float* __restrict__ part, int nchunks, int F, int cpitch, double* __restrict__ S) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= F * F) return;
  const int i = e / F, j = e - i * F;
  const int a = min(i, j), b = max(i, j);          // one triangle, mirrored: S is symmetric bit for bit
  S[e] = lp_fold(part + (int64_t)a * cpitch + b, (int64_t)F * cpitch, nchunks);
}

// workgroups 0 .. nb - 1: G; workgroup nb: loss[t]
__global__ __launch_bounds__(256) void lp_fold_kernel(const float* __restrict__ part, int nchunks, int N, int L, int C, int Cp, double l2,
                                                      const double* __restrict__ W, double* __restrict__ G, const double* __restrict__ part_loss,
                                                      int ntiles, double* __restrict__ loss, const int32_t* __restrict__ state, int nb) {
  __shared__ double sp[256];
  const int tid = threadIdx.x, F = L + 1;
  if ((int)blockIdx.x < nb) {
    const int e = blockIdx.x * 256 + tid;
    if (e >= F * C) return;
    const int f = e / C, c = e - f * C;
    const double mean = lp_fold(part + (int64_t)f * Cp + c, (int64_t)F * Cp, nchunks) / (double)N;
    G[e] = f < L ? mean + l2 * W[e] : mean;
    return;
  }
  double s = 0.0, q = 0.0;
  for (int i = tid; i < ntiles; i += 256) s += part_loss[i];            // thread t: the tiles t, t + 256, ...; then the threads in order
  for (int i = tid; i < L * C; i += 256) q += W[i] * W[i];
  const double tot = block_sum_ordered(s, sp);
  const double reg = block_sum_ordered(q, sp);
  if (tid == 0) loss[state[0]] = tot / (double)N + (0.5 * l2) * reg;
}

// W <- W - P G: a workgroup owns 4 rows of W and all classes; P's rows and G go through LDS 64 values of j at a time, thread (row, class)
// adds its products in ascending j.  Workgroup 0 first: gmax_t, the trajectory index moves on.
constexpr int ST_J = 64, ST_R = 4;
__global__ __launch_bounds__(256) void lp_step_kernel(const double* __restrict__ P, const double* __restrict__ G, double* __restrict__ W, int L, int C,
                                                      int do_step, double* __restrict__ gmax, int32_t* __restrict__ state) {
  __shared__ double sm[256];
  __shared__ double sG[ST_J * 64];
  __shared__ double sP[ST_R * ST_J];
  const int tid = threadIdx.x, F = L + 1;
  if (blockIdx.x == 0) {                           // no other workgroup looks at the state
    double mx = 0.0;
    for (int i = tid; i < F * C; i += 256) mx = fmax(mx, fabs(G[i]));
    sm[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {            // a maximum: the tree's shape does not matter
      if (tid < o) sm[tid] = fmax(sm[tid], sm[tid + o]);
      __syncthreads();
    }
    if (tid == 0) {
      const int t = state[0];
      gmax[t] = sm[0];
      state[0] = t + 1;
    }
  }
  if (!do_step) return;
  const int il = tid >> 6, c = tid & 63, i0 = blockIdx.x * ST_R, i = i0 + il;
  const bool act = i < F && c < C;
  double s = 0.0;
  for (int j0 = 0; j0 < F; j0 += ST_J) {
    const int nj = min(ST_J, F - j0);
    __syncthreads();                               // the previous slice is used up
    for (int e = tid; e < nj * C; e += 256) {
      const int jj = e / C, cc = e - jj * C;
      sG[jj * 64 + cc] = G[(int64_t)j0 * C + e];
    }
    for (int e = tid; e < ST_R * nj; e += 256) {
      const int r = e / nj, jj = e - r * nj;
      sP[r * ST_J + jj] = i0 + r < F ? P[(int64_t)(i0 + r) * F + j0 + jj] : 0.0;
    }
    __syncthreads();
    if (act)
      for (int jj = 0; jj < nj; ++jj) s += sP[il * ST_J + jj] * sG[jj * 64 + c];   // ascending j
  }
  if (act) W[(int64_t)i * C + c] = W[(int64_t)i * C + c] - s;
}

__global__ void lp_state_kernel(int32_t* state, int resume) {
  if (threadIdx.x == 0 && blockIdx.x == 0) state[0] = resume ? max(state[0] - 1, 0) : 0;
}

__global__ __launch_bounds__(256) void lp_mean_kernel(const double* __restrict__ part_loss, int ntiles, int N, double* __restrict__ loss) {
  __shared__ double sp[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < ntiles; i += 256) s += part_loss[i];
  const double tot = block_sum_ordered(s, sp);
  if (threadIdx.x == 0) loss[0] = tot / (double)N;
}

struct LpLayout { int64_t r, ploss, g, part, total; int ntiles, nchunks, Cp, gpitch; };
inline LpLayout lp_layout(int64_t N, int64_t L, int64_t C) {
  LpLayout w;
  w.ntiles = (int)((N + BM - 1) / BM);
  w.nchunks = (int)((N + LP_CHUNK - 1) / LP_CHUNK);
  w.Cp = (int)((C + 15) / 16 * 16);
  w.gpitch = (int)((L + 1 + 15) / 16 * 16);
  w.r = 0;
  w.ploss = w.r + up256(N * w.Cp * 4);
  w.g = w.ploss + up256((int64_t)w.ntiles * 8);
  w.part = w.g + up256((L + 1) * C * 8);
  const int64_t wide = w.gpitch > w.Cp ? w.gpitch : w.Cp;              // the Gram pass and the fit share the partials' slab
  w.total = w.part + up256((int64_t)w.nchunks * (L + 1) * wide * 4);
  return w;
}
inline bool lp_sizes_ok(int32_t N, int32_t L, int32_t C) { return L >= 1 && L <= 512 && C >= 2 && C <= 64 && N >= 1 && N < (1 << 24); }

void lp_launch_tile(int nj, int ntiles, hipStream_t st, const LpTileArgs& g) {
  if (nj == 1) hipLaunchKernelGGL(lp_tile_kernel<1>, dim3(ntiles), dim3(256), 0, st, g);
  else if (nj == 2) hipLaunchKernelGGL(lp_tile_kernel<2>, dim3(ntiles), dim3(256), 0, st, g);
  else if (nj == 3) hipLaunchKernelGGL(lp_tile_kernel<3>, dim3(ntiles), dim3(256), 0, st, g);
  else hipLaunchKernelGGL(lp_tile_kernel<4>, dim3(ntiles), dim3(256), 0, st, g);
}

}  // namespace

extern "C" int sv_linprobe_chunk_rows(void) { return LP_CHUNK; }

extern "C" int sv_linprobe_workspace_bytes(int32_t N, int32_t L, int32_t C, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  if (!lp_sizes_ok(N, L, C)) return SV_E_UNSUPPORTED;
  *bytes = lp_layout(N, L, C).total;
  return SV_OK;
}

extern "C" int sv_linprobe_gram(const float* x, int32_t ldx, int32_t N, int32_t L, double* S, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  if (!x || !S || !workspace) return SV_E_BADARG;
  if (!al(x, 4) || !al(S, 8) || !al(workspace, 16)) return SV_E_BADARG;
  if (!lp_sizes_ok(N, L, 2) || ldx < L) return SV_E_UNSUPPORTED;
  const LpLayout w = lp_layout(N, L, 2);           // the slab of partials does not depend on C
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)((char*)workspace + w.part);
  const int F = L + 1, nff = (F + 15) / 16;
  hipLaunchKernelGGL(lp_atb_kernel, dim3(w.nchunks, (nff + 3) / 4, (nff + 3) / 4), dim3(256), 0, st, x, ldx, N, L, (const float*)nullptr, 0, F,
                     w.gpitch, part);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(lp_gram_fold_kernel, dim3((F * F + 255) / 256), dim3(256), 0, st, (const float*)part, w.nchunks, F, w.gpitch, S);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_linprobe_fit(const float* x, int32_t ldx, const uint8_t* y, int32_t N, int32_t L, int32_t C, const double* P, double l2,
                               int32_t iters, int32_t resume, double* W, double* loss, double* gmax, double* grad, int32_t* state,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !y || !P || !W || !loss || !gmax || !state || !workspace) return SV_E_BADARG;
  if (!al(x, 4) || !al(P, 8) || !al(W, 8) || !al(loss, 8) || !al(gmax, 8) || !al(grad, 8) || !al(state, 4) || !al(workspace, 16)) return SV_E_BADARG;
  if (!lp_sizes_ok(N, L, C) || ldx < L || iters < 0 || (resume != 0 && resume != 1) || !(l2 >= 0.0) || l2 > 1.79769313486231570815e308)
    return SV_E_UNSUPPORTED;
  const LpLayout w = lp_layout(N, L, C);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)(ws + w.part);
  double* G = grad ? grad : (double*)(ws + w.g);
  LpTileArgs g = {};
  g.x = x; g.cls = y; g.w = W; g.r = (float*)(ws + w.r); g.part_loss = (double*)(ws + w.ploss);
  g.ldx = ldx; g.N = N; g.L = L; g.C = C; g.Cp = w.Cp; g.vecx = !(ldx & 3) && al(x, 16); g.predict = 0;
  const int F = L + 1, nff = (F + 15) / 16, nb = (F * C + 255) / 256;
  hipLaunchKernelGGL(lp_state_kernel, dim3(1), dim3(64), 0, st, state, resume);
  SV_LAUNCH_CHECK();
  for (int it = 0; it <= iters; ++it) {
    lp_launch_tile(w.Cp / 16, w.ntiles, st, g);
    SV_LAUNCH_CHECK();
    hipLaunchKernelGGL(lp_atb_kernel, dim3(w.nchunks, (nff + 3) / 4, 1), dim3(256), 0, st, x, ldx, N, L, (const float*)g.r, w.Cp, w.Cp, w.Cp, part);
    SV_LAUNCH_CHECK();
    hipLaunchKernelGGL(lp_fold_kernel, dim3(nb + 1), dim3(256), 0, st, (const float*)part, w.nchunks, N, L, C, w.Cp, l2, (const double*)W, G,
                       (const double*)g.part_loss, w.ntiles, loss, (const int32_t*)state, nb);
    SV_LAUNCH_CHECK();
    const int do_step = it < iters;
    hipLaunchKernelGGL(lp_step_kernel, dim3(do_step ? (F + ST_R - 1) / ST_R : 1), dim3(256), 0, st, P, (const double*)G, W, L, C, do_step, gmax, state);
    SV_LAUNCH_CHECK();
  }
  return SV_OK;
}

extern "C" int sv_linprobe_predict(const float* q, int32_t ldq, int32_t Nq, int32_t L, int32_t C, const double* W, int32_t* pred,
                                   const uint8_t* q_class, int64_t* acc, double* loss, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!q || !W || !pred || !workspace || (loss && !q_class)) return SV_E_BADARG;
  if (!al(q, 4) || !al(W, 8) || !al(pred, 4) || !al(acc, 8) || !al(loss, 8) || !al(workspace, 16)) return SV_E_BADARG;
  if (!lp_sizes_ok(Nq, L, C) || ldq < L) return SV_E_UNSUPPORTED;
  const LpLayout w = lp_layout(Nq, L, C);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  LpTileArgs g = {};
  g.x = q; g.cls = q_class; g.w = W; g.part_loss = (double*)(ws + w.ploss); g.pred = pred; g.acc = (unsigned long long*)acc;
  g.ldx = ldq; g.N = Nq; g.L = L; g.C = C; g.Cp = w.Cp; g.vecx = !(ldq & 3) && al(q, 16); g.predict = 1;
  lp_launch_tile(w.Cp / 16, w.ntiles, st, g);
  SV_LAUNCH_CHECK();
  if (loss) {
    hipLaunchKernelGGL(lp_mean_kernel, dim3(1), dim3(256), 0, st, (const double*)g.part_loss, w.ntiles, Nq, loss);
    SV_LAUNCH_CHECK();
  }
  return SV_OK;
}
