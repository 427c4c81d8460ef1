// Host emulation of the device eigensolver's kernels (gpras_amd/csrc/eig_jacobi.h), for tests/test_eigh_emulation.py: the kernel
// source itself is compiled for the CPU and run with one std::thread per work-item.  A workgroup is 256 threads and a std::barrier
// (__syncthreads); the workgroups of a launch run one after the other; LDS is static storage; v_mfma_f64_16x16x4_f64 is
// reproduced from its lane layout (lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] and holds D[(l >> 4) + 4 q][l & 15]).
// The test rewrites three tokens of the header into "eig_emu.h" (the include of gprx_common.h, the dynamic-LDS declaration, the
// MFMA builtin); everything else, the host driver included, is the code the GPU runs.  It checks indexing, barriers, the
// schedule, bounds and the arithmetic's accuracy; it says nothing about speed or about the hardware.
//   usage: emu n in.bin out.bin     in: n * n doubles (row-major); out: lam (n) then V (n * n)
#include <barrier>
#include <thread>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cstdint>
#include <cmath>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
thread_local dim3 threadIdx, blockIdx;
static std::barrier<>* g_bar;
static double g_dyn[20000];
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
inline void __syncthreads() { g_bar->arrive_and_wait(); }
typedef double d4 __attribute__((ext_vector_type(4)));
typedef int hipStream_t; typedef int hipError_t; enum { hipSuccess = 0, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipFuncAttributeMaxDynamicSharedMemorySize };
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t b, int, hipStream_t) { memcpy(d, s, b); return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return 0; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
static double sa[4][64], sb[4][64];
inline d4 emu_mfma(double a, double b, d4 c, int, int, int) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  sa[wave][lane] = a; sb[wave][lane] = b;
  __syncthreads();
  for (int q = 0; q < 4; ++q) {
    const int i = (lane >> 4) + 4 * q, j = lane & 15;
    double s = c[q];
    for (int k = 0; k < 4; ++k) s += sa[wave][k * 16 + i] * sb[wave][k * 16 + j];
    c[q] = s;
  }
  __syncthreads();
  return c;
}
template <class K, class... Args>
void launch(K kernel, dim3 grid, dim3 block, Args... args) {
  std::barrier<> bar(block.x);
  g_bar = &bar;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < block.x; ++t)
    th.emplace_back([=, &bar]() {
      for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
          threadIdx = dim3(t); blockIdx = dim3(bx, by);
          kernel(args...);
          bar.arrive_and_wait();
        }
    });
  for (auto& x : th) x.join();
}
#define hipLaunchKernelGGL(k, g, b, sm, st, ...) launch(k, g, b, __VA_ARGS__)
#include "eig_emu.h"
using namespace gprx;
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int n = atoi(argv[1]);
  const int lda = n + 3;  // padding columns hold a sentinel that must survive
  std::vector<double> A((size_t)n * lda, 1e300), V((size_t)n * n), lam(n), ws(eig_layout(n).total), g((size_t)n * n);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(g.data(), 8, g.size(), f) != g.size()) return 2;
  fclose(f);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) A[(size_t)i * lda + j] = g[(size_t)i * n + j];
  int sweeps = -1, status = -1;
  double off = -1;
  eig_jacobi_run_impl(0, n, A.data(), lda, V.data(), n, lam.data(), ws.data(), &sweeps, &off, &status);
  int padding_written = 0;
  for (int i = 0; i < n; ++i)
    for (int j = n; j < lda; ++j) padding_written += A[(size_t)i * lda + j] != 1e300;
  printf("%d %d %.17g %d\n", status, sweeps, off, padding_written);
  f = fopen(argv[3], "wb");
  fwrite(lam.data(), 8, n, f);
  fwrite(V.data(), 8, V.size(), f);
  fclose(f);
  return 0;
}
