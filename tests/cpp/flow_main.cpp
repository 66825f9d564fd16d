// zp::FlowOpts / zp::flow_aggregate through the C++ facade
// (tests/test_flows_cpp.py). Reads one frame per line (hex) from stdin, parses
// the batch on the device and prints, for three option sets,
//   <name> <F> <keyed frames> <keyed bytes> <overflow> | <flow_of ...>
// and one line per flow with the entry's 64 bytes in hex, which the test
// compares with the Python facade's.
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
    static_assert(sizeof(zp_flow_entry) == 64 && sizeof(zp_flow_key) == 40, "zero_packet.h");
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
    uint32_t* d_flow_of = nullptr;
    zp_flow_entry* d_flows = nullptr;
    uint64_t* d_count = nullptr;
    void* d_scratch = nullptr;
    const uint64_t nscratch = zp_flow_scratch_bytes(n, n);
    HIP_OK(hipMalloc((void**)&d_recs, n * sizeof(zp_record)));
    HIP_OK(hipMalloc((void**)&d_flow_of, n * 4));
    HIP_OK(hipMalloc((void**)&d_flows, n * sizeof(zp_flow_entry)));
    HIP_OK(hipMalloc((void**)&d_count, 32));
    HIP_OK(hipMalloc(&d_scratch, nscratch));
    try {
        zp::parse_batch_device(d_arena, d_offs, d_lens, n, d_recs, nullptr, nullptr);
        const std::pair<const char*, zp::FlowOpts> sets[] = {
            {"five", zp::FlowOpts(n)},
            {"bidir", zp::FlowOpts(n).bidir().vlan()},
            {"addr", zp::FlowOpts(n).ports(false).proto(false).hash_mask(3)},
        };
        for (const auto& [name, opts] : sets) {
            zp::flow_aggregate(d_arena, d_offs, d_lens, d_recs, n, opts, nullptr, d_flow_of, d_flows,
                               d_count, d_scratch, nscratch, nullptr);
            HIP_OK(hipDeviceSynchronize());
            uint64_t count[4];
            HIP_OK(hipMemcpy(count, d_count, 32, hipMemcpyDeviceToHost));
            std::vector<uint32_t> flow_of(n);
            std::vector<zp_flow_entry> flows(count[0]);
            HIP_OK(hipMemcpy(flow_of.data(), d_flow_of, 4 * n, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(flows.data(), d_flows, sizeof(zp_flow_entry) * count[0],
                             hipMemcpyDeviceToHost));
            std::printf("%s %llu %llu %llu %llu |", name, (unsigned long long)count[0],
                        (unsigned long long)count[1], (unsigned long long)count[2],
                        (unsigned long long)count[3]);
            for (uint32_t f : flow_of) std::printf(" %u", f);
            std::printf("\n");
            for (const zp_flow_entry& e : flows) {
                const uint8_t* b = reinterpret_cast<const uint8_t*>(&e);
                for (size_t k = 0; k < sizeof e; ++k) std::printf("%02x", b[k]);
                std::printf("\n");
            }
        }
        // a refusal throws with the library's text
        try {
            zp::flow_aggregate(d_arena, d_offs, d_lens, d_recs, n, zp::FlowOpts(0), nullptr, d_flow_of,
                               d_flows, d_count, d_scratch, nscratch, nullptr);
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
