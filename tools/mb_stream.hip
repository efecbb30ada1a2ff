// mb_stream.hip -- microbenchmark of streaming max-merge variants on gfx950.
// Not part of the product: used to pick the k_block_max shape.
//   mb_stream [cells]        tile size, vectors per lane, grid form, nontemporal
//   mb_stream [cells] cond   conditional-store rules on stale / fresh / sparse input
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef unsigned long long u64;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

template <int U, bool NTLD_S, bool NTST>
__global__ __launch_bounds__(256) void k_max(u64* __restrict__ s, const u64* __restrict__ d, u64 n) {
  const u64 tile = 256 * 2 * U;
  for (u64 t = blockIdx.x; t * tile < n; t += gridDim.x) {
    u64 base = t * tile + threadIdx.x * 2;
    u64x2 dv[U], sv[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      u64 i = base + u * 512;
      if (i < n) {
        dv[u] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(d + i));
        if (NTLD_S) sv[u] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(s + i));
        else sv[u] = *reinterpret_cast<const u64x2*>(s + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      u64 i = base + u * 512;
      if (i < n) {
        u64x2 r;
        r.x = dv[u].x > sv[u].x ? dv[u].x : sv[u].x;
        r.y = dv[u].y > sv[u].y ? dv[u].y : sv[u].y;
        if (NTST) __builtin_nontemporal_store(r, reinterpret_cast<u64x2*>(s + i));
        else *reinterpret_cast<u64x2*>(s + i) = r;
      }
    }
  }
}

// copy reference: 1 read + 1 write
__global__ __launch_bounds__(256) void k_copy(u64* __restrict__ s, const u64* __restrict__ d, u64 n) {
  for (u64 i = ((u64)blockIdx.x * 256 + threadIdx.x) * 2; i < n; i += (u64)gridDim.x * 512)
    *reinterpret_cast<u64x2*>(s + i) = *reinterpret_cast<const u64x2*>(d + i);
}

// ---- conditional-store variants of the product shape (1 vector per lane,
// 512-cell tile per workgroup, nontemporal): `mb_stream [cells] cond`
enum { ST_ALWAYS, ST_WAVE, ST_LINE, ST_LANE, ST_NONE };

// ST_WAVE: the wave stores its 1 KiB if any of its lanes changed.  ST_LINE:
// a lane stores if a lane of the wave in the same 128-B line of s changed
// (8 lanes x 16 B; `s` may start inside a line).  ST_LANE: per lane, leaves
// byte-masked lines.  ST_NONE: the two read streams alone (sink never true).
template <int MODE>
__global__ __launch_bounds__(256) void k_cond(u64* __restrict__ s, const u64* __restrict__ d, u64 n, u64 sink) {
  const u64 i = (u64)blockIdx.x * 512 + (u64)threadIdx.x * 2;
  const bool in = i < n;
  u64x2 dv, sv;
  if (in) {
    dv = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(d + i));
    sv = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(s + i));
  }
  const bool changed = in && (dv.x > sv.x || dv.y > sv.y);
  bool st = in;
  if (MODE == ST_WAVE) st = in && __ballot(changed) != 0;
  if (MODE == ST_LINE) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned off = (unsigned)(reinterpret_cast<uintptr_t>(s) >> 4) & 7u;
    const unsigned line = (lane + off) >> 3;
    const u64 mates = line < 8 ? (0xFFull << (8 * line)) >> off : ~0ull << (64 - off);
    st = in && (__ballot(changed) & mates) != 0;
  }
  if (MODE == ST_LANE) st = changed;
  if (MODE == ST_NONE) st = in && (dv.x ^ sv.y) == sink && (dv.y ^ sv.x) == ~sink;
  if (st) {
    u64x2 r;
    r.x = dv.x > sv.x ? dv.x : sv.x;
    r.y = dv.y > sv.y ? dv.y : sv.y;
    __builtin_nontemporal_store(r, reinterpret_cast<u64x2*>(s + i));
  }
}

__device__ inline u64 mix64(u64 x) {  // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// state in [2^10, 2^40); delta by input kind: 0 all stale (<= state), 1 fresh
// (75 % of cells advanced at random, the rest behind), 2.. sparse (equal to
// the state but for one advanced cell per 2^(kind - 2) cells)
__global__ void k_fill(u64* __restrict__ s, u64* __restrict__ d, u64 n, int kind) {
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
    const u64 h = mix64(i), v = (h >> 24) | 1024;
    const u64 step = (h & 1023) % 1000;
    u64 dv;
    if (kind == 0) dv = v - step;
    else if (kind == 1) dv = ((h >> 10) & 3) ? v + 1 + step : v - step;
    else dv = (i & ((1ull << (kind - 2)) - 1)) == 0 ? v + 1 : v;
    s[i] = v;
    d[i] = dv;
  }
}

template <int MODE>
float time_cond(u64* s, const u64* s0, const u64* d, u64 n, int reps) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  float sum = 0;
  for (int r = -1; r < reps; r++) {  // r = -1 warms up; the state is put back before every launch
    CK(hipMemcpyAsync(s, s0, n * 8, hipMemcpyDeviceToDevice, 0));
    CK(hipEventRecord(a));
    hipLaunchKernelGGL((k_cond<MODE>), dim3((unsigned)((n + 511) / 512)), dim3(256), 0, 0, s, d, n, 0x5EEDull);
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b));
    if (r >= 0) sum += ms;
  }
  CK(hipGetLastError());
  CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
  return sum / reps;
}

// one table row per input: ms per launch of every variant; `shift` cells (even)
// move s off the 128-B line grid, as an even slot0 that is no multiple of 16 does
int cond_main(u64 n) {
  const u64 pad = 16;
  u64 *sbuf, *s0, *d;
  CK(hipMalloc(&sbuf, (n + pad) * 8)); CK(hipMalloc(&s0, (n + pad) * 8)); CK(hipMalloc(&d, n * 8));
  const int kinds[] = {0, 1, 2 + 4, 2 + 7, 2 + 10, 2 + 13, 2 + 16};
  printf("cells %llu; ms per launch, and the two read streams alone (no-store) as GB/s\n", n);
  printf("%-28s %8s %8s %8s %8s %8s %8s\n", "input", "always", "wave", "line", "lane", "no-store", "rd GB/s");
  const u64 shifts[] = {0, 2};
  for (u64 shift : shifts) {
    u64 *s = sbuf + shift, *z = s0 + shift;
    for (int kind : kinds) {
      hipLaunchKernelGGL(k_fill, dim3(8192), dim3(256), 0, 0, z, d, n, kind);
      CK(hipDeviceSynchronize());
      char name[64];
      if (kind == 0) snprintf(name, sizeof name, "all stale");
      else if (kind == 1) snprintf(name, sizeof name, "fresh 75%%");
      else snprintf(name, sizeof name, "sparse 1 per 2^%d cells", kind - 2);
      char row[96];
      snprintf(row, sizeof row, "%s%s", name, shift ? " (+16 B)" : "");
      const float t0 = time_cond<ST_ALWAYS>(s, z, d, n, 3), t1 = time_cond<ST_WAVE>(s, z, d, n, 3),
                  t2 = time_cond<ST_LINE>(s, z, d, n, 3), t3 = time_cond<ST_LANE>(s, z, d, n, 3),
                  t4 = time_cond<ST_NONE>(s, z, d, n, 3);
      printf("%-28s %8.3f %8.3f %8.3f %8.3f %8.3f %8.0f\n", row, t0, t1, t2, t3, t4, 16.0 * n / 1e6 / t4);
      fflush(stdout);
    }
  }
  return 0;
}

template <typename F>
float timeit(F f, int reps) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  f();
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(a));
  for (int r = 0; r < reps; r++) f();
  CK(hipEventRecord(b));
  CK(hipEventSynchronize(b));
  float ms; CK(hipEventElapsedTime(&ms, a, b));
  return ms / reps;
}

int main(int argc, char** argv) {
  u64 n = (argc > 1 ? strtoull(argv[1], 0, 10) : (1ull << 31));  // cells
  if (argc > 2 && !strcmp(argv[2], "cond")) return cond_main(n);
  u64 *s, *d;
  CK(hipMalloc(&s, n * 8)); CK(hipMalloc(&d, n * 8));
  CK(hipMemset(s, 1, n * 8)); CK(hipMemset(d, 2, n * 8));
  const double gb = 24.0 * n / 1e9;
  int grids[] = {1024, 2048, 4096, 8192, 16384, 65536, 0};
  for (int g : grids) {
    u64 G = g ? g : (n + 2047) / 2048;
    float ms = timeit([&] { hipLaunchKernelGGL((k_max<4, false, false>), dim3(G), dim3(256), 0, 0, s, d, n); }, 5);
    printf("max U4 plain      grid %8llu: %.3f ms  %.0f GB/s\n", G, ms, gb / ms * 1e3);
  }
  for (int g : {2048, 8192, 0}) {
    u64 G1 = g ? g : (n + 1023) / 1024, G2 = g ? g : (n + 4095) / 4096;
    float ms = timeit([&] { hipLaunchKernelGGL((k_max<2, false, false>), dim3(G1), dim3(256), 0, 0, s, d, n); }, 5);
    printf("max U2            grid %8llu: %.3f ms  %.0f GB/s\n", G1, ms, gb / ms * 1e3);
    ms = timeit([&] { hipLaunchKernelGGL((k_max<8, false, false>), dim3(G2), dim3(256), 0, 0, s, d, n); }, 5);
    printf("max U8            grid %8llu: %.3f ms  %.0f GB/s\n", G2, ms, gb / ms * 1e3);
    u64 G = g ? g : (n + 2047) / 2048;
    ms = timeit([&] { hipLaunchKernelGGL((k_max<4, true, false>), dim3(G), dim3(256), 0, 0, s, d, n); }, 5);
    printf("max U4 ntld-state grid %8llu: %.3f ms  %.0f GB/s\n", G, ms, gb / ms * 1e3);
    ms = timeit([&] { hipLaunchKernelGGL((k_max<4, false, true>), dim3(G), dim3(256), 0, 0, s, d, n); }, 5);
    printf("max U4 ntst       grid %8llu: %.3f ms  %.0f GB/s\n", G, ms, gb / ms * 1e3);
    ms = timeit([&] { hipLaunchKernelGGL((k_max<4, true, true>), dim3(G), dim3(256), 0, 0, s, d, n); }, 5);
    printf("max U4 nt both    grid %8llu: %.3f ms  %.0f GB/s\n", G, ms, gb / ms * 1e3);
  }
  float ms = timeit([&] { hipLaunchKernelGGL(k_copy, dim3(8192), dim3(256), 0, 0, s, d, n); }, 5);
  printf("copy (16 B/cell)  grid 8192: %.3f ms  %.0f GB/s\n", ms, 16.0 * n / 1e9 / ms * 1e3);
  return 0;
}
