// Rate of v_exp_f32 the card sustains: independent chains of exponentials on every CU, no memory traffic.  The yardstick of
// scripts/bench_latent_dims.py (sv_latent_dims_lse issues 9 exponentials per 8 scores).
//   hipcc --offload-arch=gfx950 -O3 -o build/exp_f32_rate scripts/micro/exp_f32_rate.hip && build/exp_f32_rate
// Prints exponentials per second for 1, 2 and 4 waves per SIMD with 16 chains per lane, alone and with PLAIN fused multiply-adds
// per exponential beside them (the kernel's own mix is about 9 plain vector instructions per exponential); the last line,
// EXP_PER_S <rate>, is the best exponential-only figure.
#include <hip/hip_runtime.h>
#include <stdio.h>

template <int PLAIN>
__global__ __launch_bounds__(256) void k(float* out, int iters, float x0, float c) {
  float x[16], y[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { x[i] = x0 - (float)i * 0.01f - (float)threadIdx.x * 1e-4f; y[i] = x[i]; }
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      x[i] = __builtin_amdgcn_exp2f(x[i]);         // the chain of lane-register i: 16 independent ones per lane
#pragma unroll
      for (int p = 0; p < PLAIN; ++p) y[i] = __builtin_fmaf(y[i], c, x0);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += x[i] + y[i];
  if (s == 12345.678f) out[0] = s;
}

template <int PLAIN>
double run(int wgs_per_cu, int cus) {
  float* out;
  if (hipMalloc(&out, 4) != hipSuccess) return 0.0;
  const int iters = 4000, grid = cus * wgs_per_cu;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  k<PLAIN><<<grid, 256>>>(out, 50, -1.f, 0.999f);
  (void)hipDeviceSynchronize();
  double best = 0.0;
  for (int rep = 0; rep < 5; ++rep) {
    (void)hipEventRecord(e0);
    k<PLAIN><<<grid, 256>>>(out, iters, -1.f, 0.999f);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double rate = (double)grid * 256 * 16 * iters / (ms * 1e-3);
    if (rate > best) best = rate;
  }
  printf("v_exp_f32 + %d v_fma_f32 each  %d waves/SIMD  %.4g exponentials/s\n", PLAIN, wgs_per_cu, best);
  (void)hipFree(out);
  return best;
}

int main() {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
  const int cus = p.multiProcessorCount;
  printf("%s, %d CUs\n", p.name, cus);
  double best = 0.0;
  for (int w : {1, 2, 4}) { const double r = run<0>(w, cus); if (r > best) best = r; }
  for (int w : {2, 4}) run<4>(w, cus);
  for (int w : {2, 4}) run<9>(w, cus);
  printf("EXP_PER_S %.6g\n", best);
  return 0;
}
