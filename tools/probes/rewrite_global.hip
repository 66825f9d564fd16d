// rewrite_global.hip — lab probe: the header rewrite with the old header
// words read by plain global byte loads instead of the cooperative 16-B
// staging of zp_rewrite.hip (same per-frame code, zp_rewrite.h). No LDS, no
// wave-wide operation. tools/rewrite_bench.py --probe times it beside the
// product kernel; the slower of the two is logged as rejected.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../zero-packet_amd/csrc/zp_rewrite.h"

struct GlobalReader {
    const __attribute__((address_space(1))) uint8_t* g;
    __device__ __forceinline__ uint32_t operator()(uint32_t x) { return g[x]; }
    __device__ __forceinline__ bool has4(uint32_t) const { return false; }
    __device__ __forceinline__ uint32_t le4(uint32_t) const { return 0u; }
};

__global__ void __launch_bounds__(256)
rewrite_global_kernel(uint8_t* arena, const uint64_t* __restrict__ offs,
                      const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs,
                      uint64_t n, ColPtrs c) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const zp_u32x2 q = *(const zp_u32x2*)(recs + i);
    const uint32_t flags = q.x & ZP_F_MASK;
    const bool far = ((q.x >> 24) & 3u) == ZP_ETH_CODE_FAR;
    uint32_t hl = far ? 22u : 14u + 4u * ((q.x >> 24) & 3u);
    const uint32_t l4 = far ? q.y : q.y & ZP_L4_NEAR_MAX;
    if ((q.x >> 26) != 0 || !(flags & ZP_F_ETHERNET)) return;
    const uint32_t len = lens[i];
    typedef __attribute__((address_space(1))) uint8_t* gptr;
    const gptr g = (gptr)(arena + offs[i]);
    if (len < 14) return;
    GlobalReader rd{g};
    if (far) {
        const uint32_t t0 = rd16(rd, 12u);
        hl = t0 == 0x8100 ? 18u : t0 == 0x88A8 ? 22u : 14u;
    }
    if (len < hl) return;
    rewrite_frame(rd, g, flags, hl, l4, len, i, c);
}

extern "C" int rewrite_global(uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                              const zp_record* records, uint64_t n, const void* const* cols,
                              void* stream) {
    ColPtrs c;
    for (int k = 0; k < ZP_COL_COUNT; ++k) c.p[k] = (uint8_t*)cols[k];
    if (n == 0) return 0;
    hipLaunchKernelGGL(rewrite_global_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, arena, offs, lens, records, n, c);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
