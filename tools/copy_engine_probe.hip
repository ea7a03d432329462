// copy_engine_probe.hip -- the bare engine copy, once, before the pipeline relies on it: a kernel writes a pattern into an
// 8 MB device buffer, an event created with hipEventReleaseToSystem is recorded behind it, and when the event has passed
// ONE hsa_amd_memory_async_copy (csrc/copy_engine.h: the HSA runtime found in the process, agents from
// hsa_amd_pointer_info) moves the buffer into hipHostMalloc'ed memory; the host compares every word.
//   hipcc --offload-arch=gfx950 -O2 -I nblic-image-compression_amd/csrc -o tools/copy_engine_probe tools/copy_engine_probe.hip
// Prints "copy_engine_probe ok" and returns 0, or says what failed and returns 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "copy_engine.h"

__global__ void k_pattern(uint32_t *p, size_t n, uint32_t salt) {
    for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) p[i] = uint32_t(i) * 2654435761u ^ salt;
}

#define OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    using namespace nblic;
    const size_t bytes = size_t(8) << 20, n = bytes / sizeof(uint32_t);
    uint32_t *dev = nullptr, *host = nullptr;
    hipStream_t s; hipEvent_t released;
    OK(hipMalloc(&dev, bytes));
    OK(hipHostMalloc(&host, bytes, hipHostMallocDefault));
    for (size_t i = 0; i < n; i++) host[i] = 0xDEADBEEFu;
    OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    OK(hipEventCreateWithFlags(&released, hipEventDisableTiming | hipEventReleaseToSystem));
    CopyEngine e;
    if (!e.open()) { printf("the HSA runtime's copy entry points were not found in this process\n"); return 1; }
    uint64_t sig = 0;
    if (e.api().signal_create(0, 0, nullptr, &sig) != 0 || !sig) { printf("hsa_signal_create failed\n"); return 1; }
    EngineLane lane;
    for (auto &h : lane.sig) h = sig;
    int rc = 0;
    for (uint32_t salt = 1; salt <= 2 && rc == 0; salt++) {          // twice: the second pattern must replace the first
        hipLaunchKernelGGL(k_pattern, dim3(512), dim3(256), 0, s, dev, n, salt);
        OK(hipGetLastError());
        OK(hipEventRecord(released, s));
        OK(hipEventSynchronize(released));
        const CopyPiece pc{host, dev, bytes};
        if (!copy_detail::engine_issue(e, lane, 0, &pc, 1)) { printf("the engine copy could not be issued\n"); rc = 1; break; }
        double waited = 0;
        if (!copy_detail::wait_signal(e, sig, 0, &waited)) { printf("the engine copy did not complete\n"); rc = 1; break; }
        size_t bad = 0;
        for (size_t i = 0; i < n; i++) bad += host[i] != (uint32_t(i) * 2654435761u ^ salt);
        printf("pattern %u: %zu of %zu words differ, waited %.3f ms (agents: device %llx, host %llx)\n", salt, bad, n, waited * 1e3,
               (unsigned long long)lane.src_agent, (unsigned long long)lane.dst_agent);
        if (bad) rc = 1;
    }
    e.api().signal_destroy(sig);
    OK(hipStreamSynchronize(s));
    OK(hipEventDestroy(released)); OK(hipStreamDestroy(s)); OK(hipHostFree(host)); OK(hipFree(dev));
    if (rc == 0) printf("copy_engine_probe ok\n");
    return rc;
}
