// zp::Select / zp::select / zp::gather_frames through the C++ facade
// (tests/test_select_cpp.py). Reads one frame per line (hex) from stdin, parses
// the batch on the device and prints, for three selectors, one line
//   <name> <count> <bytes> | <idx ...> | <packed bytes of the gather, hex>
// which the test compares with the Python facade's.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "zero_packet.hpp"

#define HIP_OK(x)                                                              \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));       \
            return 2;                                                          \
        }                                                                      \
    } while (0)

template <class T>
static T* dev_copy(const std::vector<T>& v) {
    T* p = nullptr;
    if (hipMalloc((void**)&p, v.size() * sizeof(T) + 64) != hipSuccess) std::abort();
    if (hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) std::abort();
    return p;
}

int main() {
    std::vector<uint8_t> arena;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        offs.push_back(arena.size());
        lens.push_back((uint32_t)(line.size() / 2));
        for (size_t k = 0; k + 1 < line.size(); k += 2)
            arena.push_back((uint8_t)std::stoul(line.substr(k, 2), nullptr, 16));
    }
    const uint64_t n = offs.size();
    arena.resize(arena.size() + 64);
    uint8_t* d_arena = dev_copy(arena);
    uint64_t* d_offs = dev_copy(offs);
    uint32_t* d_lens = dev_copy(lens);
    zp_record* d_recs = nullptr;
    uint32_t* d_idx = nullptr;
    uint64_t *d_packed = nullptr, *d_count = nullptr, *d_out_offs = nullptr;
    uint32_t* d_out_lens = nullptr;
    uint8_t* d_dst = nullptr;
    void* d_scratch = nullptr;
    const uint64_t nscratch = zp_select_scratch_bytes(n);
    HIP_OK(hipMalloc((void**)&d_recs, n * sizeof(zp_record)));
    HIP_OK(hipMalloc((void**)&d_idx, n * 4));
    HIP_OK(hipMalloc((void**)&d_packed, n * 8));
    HIP_OK(hipMalloc((void**)&d_out_offs, n * 8));
    HIP_OK(hipMalloc((void**)&d_out_lens, n * 4));
    HIP_OK(hipMalloc((void**)&d_count, 16));
    HIP_OK(hipMalloc((void**)&d_dst, arena.size()));
    HIP_OK(hipMalloc(&d_scratch, nscratch));
    try {
        zp::parse_batch_device(d_arena, d_offs, d_lens, n, d_recs, nullptr, nullptr);
        const std::pair<const char*, zp::Select> sels[] = {
            {"tcp", zp::Select().ok().has(ZP_F_TCP)},
            {"five", zp::Select().ok().eq(ZP_COL_L4_PROTO, 17).between(ZP_COL_DEST_PORT, 1000, 40000)
                         .prefix(ZP_COL_SRC_ADDR, std::array<uint8_t, 4>{192, 168, 0, 0}, 16)
                         .eq(ZP_COL_IP_VERSION, 4)},
            {"v6", zp::Select().len(70).outside(ZP_COL_TTL, 0, 63)
                       .prefix(ZP_COL_DEST_ADDR, std::array<uint8_t, 16>{0xfe, 0x80}, 10)
                       .mac(ZP_COL_SRC_MAC, {0x34, 0x97, 0xf6, 0x94, 0x02, 0x0f})},
        };
        for (const auto& [name, sel] : sels) {
            zp::select(d_arena, d_offs, d_lens, d_recs, n, sel, nullptr, d_idx, d_packed, d_count,
                       d_scratch, nscratch, nullptr);
            zp::gather_frames(d_arena, d_offs, d_lens, d_recs, nullptr, n, d_idx, d_packed, n,
                              d_count, d_dst, arena.size(), d_out_offs, d_out_lens, nullptr, nullptr,
                              nullptr);
            HIP_OK(hipDeviceSynchronize());
            uint64_t count[2];
            HIP_OK(hipMemcpy(count, d_count, 16, hipMemcpyDeviceToHost));
            std::vector<uint32_t> idx(count[0]);
            std::vector<uint8_t> bytes(count[1]);
            HIP_OK(hipMemcpy(idx.data(), d_idx, 4 * count[0], hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(bytes.data(), d_dst, count[1], hipMemcpyDeviceToHost));
            std::printf("%s %llu %llu |", name, (unsigned long long)count[0],
                        (unsigned long long)count[1]);
            for (uint32_t i : idx) std::printf(" %u", i);
            std::printf(" | ");
            for (uint8_t b : bytes) std::printf("%02x", b);
            std::printf("\n");
        }
        // a refusal throws with the library's text
        try {
            zp::select(d_arena, d_offs, d_lens, d_recs, n, zp::Select().ok(), nullptr, d_idx,
                       nullptr, nullptr, d_scratch, nscratch, nullptr);
            std::printf("refusal: none\n");
        } catch (const std::runtime_error& e) {
            std::printf("refusal: %s\n", e.what());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
