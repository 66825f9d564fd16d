// zp_win.h — the per-frame header window of the one-lane-per-frame kernels
// (zp_fields.hip, zp_rewrite.hip): each lane's first FX_WIN bytes (from
// A & ~15) staged in LDS with 16-B loads, and a reader over it that takes
// headers past the window from global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef FX_WIN
#define FX_WIN 112                       // staged bytes per frame (from A & ~15); longer headers
                                         // (some c4 chains) read the rest from HBM. 112 vs 160:
                                         // c3 -5 %, c5 -9 %, c4 +-2 % (28 KB of LDS per workgroup
                                         // instead of 40: more workgroups per CU; r04_cols_window_ab.log)
#endif
#define FX_CH (FX_WIN / 16)
#define FX_BLOCK 256

#define FX_GLOBAL __attribute__((address_space(1)))
typedef unsigned fx_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 fx_ld16(uintptr_t a) {
    const fx_u32x4 v = *(const FX_GLOBAL fx_u32x4*)a;
    return make_uint4(v.x, v.y, v.z, v.w);
}

struct Hdr {
    const uint8_t* win;   // this lane's cells: byte b of chunk c at win[c * 16 * FX_BLOCK + b]
    const uint8_t* g;     // frame in global memory
    uint32_t shift, wlen;
    uint4 xc;             // past the window: one cached 16-B chunk ...
    uint32_t xi;          // ... and its index from A & ~15 (~0: none)
};

__device__ __forceinline__ uint32_t hb(Hdr& h, uint32_t x) {
    const uint32_t y = x + h.shift;
    if (x < h.wlen) return h.win[(y >> 4) * 16 * FX_BLOCK + (y & 15)];
    // Headers past the window (deep IPv6 chains, IP-in-IP): one 16-B load
    // per distinct chunk, the fields of a header share it.
    if ((y >> 4) != h.xi) {
        h.xi = y >> 4;
        h.xc = fx_ld16(((uintptr_t)h.g & ~(uintptr_t)15) + 16u * h.xi);
    }
    // byte y & 15 of the chunk by shifts and one select (a select chain over
    // the four dwords was lowered to a dynamically indexed scratch copy)
    const uint64_t q = (y & 8) ? (((uint64_t)h.xc.w << 32) | h.xc.z)
                               : (((uint64_t)h.xc.y << 32) | h.xc.x);
    return (uint32_t)(q >> (8 * (y & 7))) & 0xFFu;
}
// Dword z (4-aligned, from A & ~15) of the staged window.
__device__ __forceinline__ uint32_t hdw(const Hdr& h, uint32_t z) {
    return *(const uint32_t*)(h.win + (z >> 4) * 16 * FX_BLOCK + (z & 15));
}
struct HdrReader {
    Hdr& h;
    __device__ __forceinline__ uint32_t operator()(uint32_t x) { return hb(h, x); }
    __device__ __forceinline__ bool has4(uint32_t x) const { return x + 3 < h.wlen; }
    __device__ __forceinline__ uint32_t le4(uint32_t x) const {
        const uint32_t y = x + h.shift, z = y & ~3u;
        const uint32_t lo = hdw(h, z), hi = (y & 3) ? hdw(h, z + 4) : 0u;
        return __builtin_amdgcn_alignbyte(hi, lo, y & 3);
    }
};

// Stages the chunks of [A & ~15, A + wlen) of every frame of the wave
// cooperatively: in item q, lane l loads chunk (l & 7) of frame 8q + (l >> 3)
// of its wave, so one load instruction reads eight whole 128-B windows instead
// of 64 scattered 16-B pieces. Cell (chunk c, frame t) lives at
// win[c * FX_BLOCK + t]. ga = this lane's frame address, len = its length (0:
// nothing staged); h.shift and h.wlen are set. Every lane of the wave must
// call it (ds_bpermute reads every lane).
__device__ __forceinline__ void fx_stage(uint4* win, uintptr_t ga, uint32_t len, const Hdr& h) {
    const uint32_t lane = threadIdx.x & 63, wbase = threadIdx.x & ~63u;
    const uint32_t nch = len ? (h.wlen + h.shift + 15) >> 4 : 0u;
    const uintptr_t a0 = ga & ~(uintptr_t)15;
    const uint32_t a_lo = (uint32_t)a0, a_hi = (uint32_t)(a0 >> 32);
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) {
        const uint32_t f = 8 * q + (lane >> 3);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(f << 2), (int)a_lo);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(f << 2), (int)a_hi);
        const uint32_t nc = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(f << 2), (int)nch);
        // windows past 128 B: further rounds of 8 chunks per frame
#pragma unroll
        for (uint32_t g = 0; g < (FX_CH + 7) / 8; ++g) {
            const uint32_t ch = 8 * g + (lane & 7);
            if (ch < nc && ch < FX_CH)
                win[ch * FX_BLOCK + wbase + f] =
                    fx_ld16((((uintptr_t)hi << 32) | lo) + 16u * ch);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
