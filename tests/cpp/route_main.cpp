// zp::RouteTable / zp::route through the C++ facade
// (tests/test_routes_cpp.py). Reads one frame per line (hex) from stdin,
// parses the batch on the device and prints, for two tables and both address
// columns, one line
//   <name> <col> <status> | <value_of ...> | <mask words ...>
// which the test compares with the Python facade's and tests/route_ref.py,
// with a host lookup line, then two refusal lines.
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
    const uint64_t n = offs.size(), words = (n + 63) / 64;
    arena.resize(arena.size() + 64);
    uint8_t* d_arena = dev_copy(arena);
    uint64_t* d_offs = dev_copy(offs);
    uint32_t* d_lens = dev_copy(lens);
    zp_record* d_recs = nullptr;
    uint32_t* d_value = nullptr;
    uint64_t *d_mask = nullptr, *d_status = nullptr;
    HIP_OK(hipMalloc((void**)&d_recs, n * sizeof(zp_record)));
    HIP_OK(hipMalloc((void**)&d_value, n * 4));
    HIP_OK(hipMalloc((void**)&d_mask, words * 8));
    HIP_OK(hipMalloc((void**)&d_status, 8));
    try {
        zp::parse_batch_device(d_arena, d_offs, d_lens, n, d_recs, nullptr, nullptr);
        using RT = zp::RouteTable;
        const std::pair<const char*, std::vector<zp_route_prefix>> tables[] = {
            {"fib",
             {RT::v4({192, 168, 0, 0}, 16, 1), RT::v4({192, 168, 1, 0}, 24, 2),
              RT::v4({192, 168, 1, 2}, 32, 3), RT::v4({10, 0, 0, 0}, 8, 4), RT::v4({0, 0, 0, 0}, 0, 5),
              RT::v6({0xfe, 0x80}, 10, 10),
              RT::v6({0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0x02, 0x02, 0xb3, 0xff, 0xfe, 0x1e, 0x83, 0x29}, 128, 11),
              RT::v6({0xfc, 0x00, 0x00, 0x02}, 32, 12),
              RT::v6({0xfc, 0x00, 0x00, 0x02, 0, 0, 0x00, 0x05}, 64, 13), RT::v6({0x00, 0x02}, 16, 14),
              RT::v6({0x0a}, 8, 15)}},
            {"halves", {RT::v4({0, 0, 0, 0}, 1, 7), RT::v6({0x80}, 1, 8), RT::v6({0x20}, 3, 9)}},
        };
        for (const auto& [name, prefixes] : tables) {
            const RT table(prefixes);
            void* d_table = nullptr;
            HIP_OK(hipMalloc(&d_table, table.bytes()));
            HIP_OK(hipMemcpy(d_table, table.data(), table.bytes(), hipMemcpyHostToDevice));
            for (int col : {ZP_COL_DEST_ADDR, ZP_COL_SRC_ADDR}) {
                zp::route(d_arena, d_offs, d_lens, d_recs, n, table, d_table, col, nullptr, d_value,
                          d_mask, d_status, nullptr);
                HIP_OK(hipDeviceSynchronize());
                uint64_t status = 0;
                std::vector<uint32_t> value(n);
                std::vector<uint64_t> mask(words);
                HIP_OK(hipMemcpy(&status, d_status, 8, hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(value.data(), d_value, 4 * n, hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(mask.data(), d_mask, 8 * words, hipMemcpyDeviceToHost));
                std::printf("%s %s %llu |", name, col == ZP_COL_DEST_ADDR ? "dest_addr" : "src_addr",
                            (unsigned long long)status);
                for (uint32_t v : value) std::printf(" %u", v);
                std::printf(" |");
                for (uint64_t m : mask) std::printf(" %llu", (unsigned long long)m);
                std::printf("\n");
            }
            if (std::string(name) == "fib")
                std::printf("lookup: %u %u %u %u\n", table.lookup(std::array<uint8_t, 4>{192, 168, 1, 2}),
                            table.lookup(std::array<uint8_t, 4>{11, 0, 0, 0}),
                            table.lookup(std::array<uint8_t, 16>{0xfc, 0x00, 0x00, 0x02, 0, 0, 0, 5, 1}),
                            table.lookup(std::array<uint8_t, 16>{0x30}));
            HIP_OK(hipFree(d_table));
        }
        // refusals throw with the library's text
        try {
            const RT table({RT::v4({10, 0, 0, 1}, 8, 1)});
            std::printf("refusal: none\n");
        } catch (const std::invalid_argument& e) {
            std::printf("refusal: %s\n", e.what());
        }
        try {
            const RT table({RT::v4({10, 0, 0, 0}, 8, 1)});
            zp::route(d_arena, d_offs, d_lens, d_recs, n, table, d_recs, ZP_COL_DEST_ADDR, nullptr,
                      d_value, d_mask, nullptr, nullptr);
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
