// zp::RuleTable / zp::classify through the C++ facade
// (tests/test_classify_cpp.py). Reads one frame per line (hex) from stdin,
// parses the batch on the device and prints, for three tables, one line
//   <name> <status> | <rule_of ...> | <packets:bytes ...>
// which the test compares with the Python facade's and tests/classify_ref.py,
// then one refusal line.
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
    uint32_t* d_rule = nullptr;
    zp_rule_hits* d_hits = nullptr;
    uint64_t* d_status = nullptr;
    void* d_table = nullptr;
    HIP_OK(hipMalloc((void**)&d_recs, n * sizeof(zp_record)));
    HIP_OK(hipMalloc((void**)&d_rule, n * 4));
    HIP_OK(hipMalloc((void**)&d_hits, (ZP_CLASSIFY_MAX_RULES + 1) * sizeof(zp_rule_hits)));
    HIP_OK(hipMalloc((void**)&d_status, 8));
    HIP_OK(hipMalloc(&d_table, zp_classify_table_bytes(ZP_CLASSIFY_MAX_RULES)));
    try {
        zp::parse_batch_device(d_arena, d_offs, d_lens, n, d_recs, nullptr, nullptr);
        std::vector<zp::Select> nested;
        for (uint32_t r = 0; r < 70; ++r)
            nested.push_back(zp::Select().between(ZP_COL_SRC_PORT, (69 - r) * 936, 65535));
        const std::pair<const char*, std::vector<zp::Select>> tables[] = {
            {"acl",
             {zp::Select().ok().has(ZP_F_TCP).eq(ZP_COL_DEST_PORT, 43424),
              zp::Select().ok().eq(ZP_COL_L4_PROTO, 17).between(ZP_COL_DEST_PORT, 1000, 40000)
                  .prefix(ZP_COL_SRC_ADDR, std::array<uint8_t, 4>{192, 168, 0, 0}, 16)
                  .eq(ZP_COL_IP_VERSION, 4),
              zp::Select().len(70).outside(ZP_COL_TTL, 0, 63)
                  .prefix(ZP_COL_DEST_ADDR, std::array<uint8_t, 16>{0xfe, 0x80}, 10),
              zp::Select().ok().has(ZP_F_TCP), zp::Select().ok(false)}},
            {"records", {zp::Select().has(ZP_F_TCP), zp::Select().has(ZP_F_UDP).len(0, 120),
                         zp::Select().ok(false)}},
            {"nested", nested},
        };
        for (const auto& [name, rules] : tables) {
            const zp::RuleTable table(rules);
            HIP_OK(hipMemcpy(d_table, table.data(), table.bytes(), hipMemcpyHostToDevice));
            HIP_OK(hipMemset(d_hits, 0, (table.nrules() + 1) * sizeof(zp_rule_hits)));
            zp::classify(d_arena, d_offs, d_lens, d_recs, n, table, d_table, nullptr, d_rule, d_hits,
                         nullptr, d_status, nullptr);
            HIP_OK(hipDeviceSynchronize());
            uint64_t status = 0;
            std::vector<uint32_t> rule(n);
            std::vector<zp_rule_hits> hits(table.nrules() + 1);
            HIP_OK(hipMemcpy(&status, d_status, 8, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(rule.data(), d_rule, 4 * n, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(hits.data(), d_hits, hits.size() * sizeof(zp_rule_hits),
                             hipMemcpyDeviceToHost));
            std::printf("%s %d %llu |", name, (int)table.needs_frames(), (unsigned long long)status);
            for (uint32_t r : rule) std::printf(" %u", r);
            std::printf(" |");
            for (const zp_rule_hits& h : hits)
                std::printf(" %llu:%llu", (unsigned long long)h.packets, (unsigned long long)h.bytes);
            std::printf("\n");
        }
        // a refusal throws with the library's text
        try {
            const zp::RuleTable table({zp::Select().ok()});
            zp::classify(d_arena, d_offs, d_lens, d_recs, n, table, d_table, nullptr, d_rule, d_hits,
                         nullptr, nullptr, nullptr);
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
