// Which runtime calls of a scene install wait for a busy device? One wave
// waits a bounded `ms` of the 100 MHz real-time clock on stream A; meanwhile
// the host times, one call per round, each call an install makes, on stream B
// or on no stream. A call that returns in microseconds overlaps frames in
// flight; one that takes about `ms` drains the device.
//   hipcc --offload-arch=gfx950 -O2 scripts/alloc_probe.hip -o scripts/alloc_probe && scripts/alloc_probe [ms]
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));          \
            return 1;                                                             \
        }                                                                         \
    } while (0)

__global__ void stall_kernel(unsigned long long ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

__global__ void touch_kernel(int* p) { p[threadIdx.x] = threadIdx.x; }

int main(int argc, char** argv)
{
    const int ms = argc > 1 ? std::atoi(argv[1]) : 50;
    if (ms < 1 || ms > 1000) return 2;
    hipStream_t a, b;
    CHECK(hipStreamCreateWithFlags(&a, hipStreamNonBlocking));
    CHECK(hipStreamCreateWithFlags(&b, hipStreamNonBlocking));
    const size_t bytes = 1 << 20;
    void *spare = nullptr, *buf = nullptr;
    int h[64];
    CHECK(hipMalloc(&buf, bytes));
    const char* names[] = {"hipMalloc 1 MiB", "hipFree 1 MiB", "kernel + hipStreamSynchronize on B",
                           "hipMemcpyAsync D2H 256 B + hipStreamSynchronize on B", "hipMemcpy D2H 256 B (no stream)",
                           "hipMemcpy H2D 256 B (no stream)", "hipMemsetAsync + hipStreamSynchronize on B"};
    for (int k = 0; k < 7; k++) {
        if (k == 1) CHECK(hipMalloc(&spare, bytes));
        CHECK(hipDeviceSynchronize());
        stall_kernel<<<1, 64, 0, a>>>((unsigned long long)ms * 100000ull);
        CHECK(hipGetLastError());
        const auto t0 = std::chrono::steady_clock::now();
        switch (k) {
        case 0: CHECK(hipMalloc(&spare, bytes)); break;
        case 1: CHECK(hipFree(spare)); spare = nullptr; break;
        case 2: touch_kernel<<<1, 64, 0, b>>>((int*)buf); CHECK(hipStreamSynchronize(b)); break;
        case 3: CHECK(hipMemcpyAsync(h, buf, sizeof h, hipMemcpyDeviceToHost, b)); CHECK(hipStreamSynchronize(b)); break;
        case 4: CHECK(hipMemcpy(h, buf, sizeof h, hipMemcpyDeviceToHost)); break;
        case 5: CHECK(hipMemcpy(buf, h, sizeof h, hipMemcpyHostToDevice)); break;
        case 6: CHECK(hipMemsetAsync(buf, 0, bytes, b)); CHECK(hipStreamSynchronize(b)); break;
        }
        const double call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        CHECK(hipStreamSynchronize(a));
        std::printf("{\"call\": \"%s\", \"ms\": %.3f, \"stall_ms\": %d, \"drains\": %s}\n", names[k], call_ms, ms,
                    call_ms > 0.5 * ms ? "true" : "false");
        if (k == 0) { CHECK(hipFree(spare)); spare = nullptr; }
    }
    CHECK(hipFree(buf));
    CHECK(hipStreamDestroy(a));
    CHECK(hipStreamDestroy(b));
    return 0;
}
