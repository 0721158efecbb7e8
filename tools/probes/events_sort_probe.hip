// What the payload of the event-log sort costs (wrmf_events.hip): rocprim::radix_sort_pairs over n keys of
// `bits` key bits with a payload of 4 bytes (the event index: values and timestamps are gathered afterwards), 12 bytes (index +
// value) or 20 bytes (index + value + timestamp riding through every pass).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probes/events_sort_probe.hip -o tools/probes/events_sort_probe
//   tools/probes/events_sort_probe [n = 650000000] [bits = 44]
// prints one line per payload: milliseconds (median of 3 after a warm-up) and bytes of sort buffers per event.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); std::exit(1); } } while (0)

struct Pay12 { uint32_t idx; uint32_t v[2]; };
struct Pay20 { uint32_t idx; uint32_t v[2]; uint32_t t[2]; };

template <class K>
__global__ void fill_keys(K* keys, size_t n, int bits) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    unsigned long long z = (e + 1) * 0x9E3779B97F4A7C15ull;   // splitmix64's mixer: keys spread over all the bits in use
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    keys[e] = (K)(bits >= 64 ? z : (z & ((1ull << bits) - 1)));
  }
}

template <class K, class P>
void run(size_t n, int bits, const char* name) {
  K *k0, *k1;
  P *p0, *p1;
  CHECK(hipMalloc(&k0, n * sizeof(K))); CHECK(hipMalloc(&k1, n * sizeof(K)));
  CHECK(hipMalloc(&p0, n * sizeof(P))); CHECK(hipMalloc(&p1, n * sizeof(P)));
  CHECK(hipMemset(p0, 0, n * sizeof(P)));
  hipLaunchKernelGGL(fill_keys<K>, dim3(4096), dim3(256), 0, 0, k0, n, bits);
  CHECK(hipGetLastError());
  size_t tmp_bytes = 0;
  void* tmp = nullptr;
  CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, k0, k1, p0, p1, n, 0, bits, 0));
  CHECK(hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16));
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
  float ms[4];
  for (int r = 0; r < 4; r++) {
    CHECK(hipEventRecord(a, 0));
    CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, k0, k1, p0, p1, n, 0, bits, 0));
    CHECK(hipEventRecord(b, 0));
    CHECK(hipEventSynchronize(b));
    CHECK(hipEventElapsedTime(&ms[r], a, b));
  }
  std::sort(ms + 1, ms + 4);
  std::printf("{\"payload\": \"%s\", \"n\": %zu, \"key_bits\": %d, \"key_bytes\": %zu, \"payload_bytes\": %zu, \"ms\": %.3f, \"sort_buffer_bytes_per_event\": %zu}\n",
              name, n, bits, sizeof(K), sizeof(P), ms[2], 2 * (sizeof(K) + sizeof(P)));
  std::fflush(stdout);
  CHECK(hipFree(k0)); CHECK(hipFree(k1)); CHECK(hipFree(p0)); CHECK(hipFree(p1)); CHECK(hipFree(tmp));
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? (size_t)std::atof(argv[1]) : 650000000;
  const int bits = argc > 2 ? std::atoi(argv[2]) : 44;
  if (bits <= 32) {
    run<uint32_t, uint32_t>(n, bits, "index");
    run<uint32_t, Pay12>(n, bits, "index + value");
    run<uint32_t, Pay20>(n, bits, "index + value + timestamp");
  } else {
    run<uint64_t, uint32_t>(n, bits, "index");
    run<uint64_t, Pay12>(n, bits, "index + value");
    run<uint64_t, Pay20>(n, bits, "index + value + timestamp");
  }
  return 0;
}
