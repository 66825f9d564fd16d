// zp::FlowTable through the C++ facade (tests/test_flow_table_cpp.py). Reads
// one frame per line (hex) from stdin, parses the batch on the device, runs two
// updates (the first third of the frames, then the rest) and one retire
// (max_idle 1, tcp_any FIN | RST), and prints
//   update <the 8 count words> | <flow_of ...>          twice
//   retire <F'> <retired> | <remap of the old F ...>
//   one line per retired entry, then one per surviving entry, 64 bytes in hex
//   refusal: <the library's text>
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

static void print_entries(const std::vector<zp_flow_state>& v) {
    for (const zp_flow_state& e : v) {
        const uint8_t* b = reinterpret_cast<const uint8_t*>(&e);
        for (size_t k = 0; k < sizeof e; ++k) std::printf("%02x", b[k]);
        std::printf("\n");
    }
}

int main() {
    static_assert(sizeof(zp_flow_state) == 64 && sizeof(zp_flow_key) == 40, "zero_packet.h");
    zp_flow_state probe{};
    probe.packets_flags = 0x1200000000000005ull;
    if (ZP_FLOW_STATE_PACKETS(probe) != 5 || ZP_FLOW_STATE_TCP_FLAGS(probe) != 0x12) return 3;
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
    const uint64_t n = offs.size(), cut = n / 3;
    arena.resize(arena.size() + 64);
    uint8_t* d_arena = dev_copy(arena);
    uint64_t* d_offs = dev_copy(offs);
    uint32_t* d_lens = dev_copy(lens);
    const zp::FlowOpts opts = zp::FlowOpts(n).bidir();
    const uint64_t ntable = zp::FlowTable::table_bytes(opts);
    zp_record* d_recs = nullptr;
    uint32_t *d_flow_of = nullptr, *d_remap = nullptr;
    zp_flow_state *d_flows = nullptr, *d_retired = nullptr;
    uint64_t* d_count = nullptr;
    void *d_table = nullptr, *d_scratch = nullptr;
    HIP_OK(hipMalloc((void**)&d_recs, n * sizeof(zp_record)));
    HIP_OK(hipMalloc((void**)&d_flow_of, n * 4));
    HIP_OK(hipMalloc((void**)&d_remap, n * 4));
    HIP_OK(hipMalloc((void**)&d_flows, n * sizeof(zp_flow_state)));
    HIP_OK(hipMalloc((void**)&d_retired, n * sizeof(zp_flow_state)));
    HIP_OK(hipMalloc((void**)&d_count, 64));
    HIP_OK(hipMalloc(&d_table, ntable));
    try {
        zp::FlowTable table(opts, d_table, ntable, d_flows);
        uint64_t nscratch = zp::FlowTable::update_scratch_bytes(n);
        if (table.retire_scratch_bytes() > nscratch) nscratch = table.retire_scratch_bytes();
        HIP_OK(hipMalloc(&d_scratch, nscratch));
        zp::parse_batch_device(d_arena, d_offs, d_lens, n, d_recs, nullptr, nullptr);
        table.init(nullptr);
        uint64_t count[8];
        const uint64_t parts[2][2] = {{0, cut}, {cut, n}};
        for (const auto& p : parts) {
            const uint64_t lo = p[0], m = p[1] - p[0];
            table.update(d_arena, d_offs + lo, d_lens + lo, d_recs + lo, m, nullptr, d_flow_of, d_count,
                         d_scratch, nscratch, nullptr);
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(count, d_count, 64, hipMemcpyDeviceToHost));
            std::vector<uint32_t> flow_of(m);
            HIP_OK(hipMemcpy(flow_of.data(), d_flow_of, 4 * m, hipMemcpyDeviceToHost));
            std::printf("update");
            for (uint64_t c : count) std::printf(" %llu", (unsigned long long)c);
            std::printf(" |");
            for (uint32_t f : flow_of) std::printf(" %u", f);
            std::printf("\n");
        }
        const uint64_t f_old = count[0];
        table.retire(1, 0x05, d_retired, d_remap, d_count, d_scratch, nscratch, nullptr);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(count, d_count, 16, hipMemcpyDeviceToHost));
        std::vector<uint32_t> remap(f_old);
        std::vector<zp_flow_state> retired(count[1]), flows(count[0]);
        HIP_OK(hipMemcpy(remap.data(), d_remap, 4 * f_old, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(retired.data(), d_retired, sizeof(zp_flow_state) * count[1], hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(flows.data(), table.flows(), sizeof(zp_flow_state) * count[0], hipMemcpyDeviceToHost));
        std::printf("retire %llu %llu |", (unsigned long long)count[0], (unsigned long long)count[1]);
        for (uint32_t f : remap) std::printf(" %u", f);
        std::printf("\n");
        print_entries(retired);
        print_entries(flows);
        // a refusal throws with the library's text
        try {
            zp::FlowTable small(opts, d_table, ntable - 1, d_flows);
            small.init(nullptr);
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
