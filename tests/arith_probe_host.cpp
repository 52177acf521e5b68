// tests/arith_probe_host.cpp -- the HOST branch of every probe of csrc/arith_probe.cuh (driven by tests/test_arith_model.py; built with -fsanitize=address,undefined).
//
//   arith_probe_host --list            one line "id nin nout quad" per operation of ZK_PROBE_OPS
//   arith_probe_host CASES OUT         CASES: records of little-endian 32-bit words {op, n_cases, n_cases x nin input words}; OUT: n_cases x nout words per record
//
// The bodies are the ones capi_probe.hip compiles for the device, so a later disagreement on the GPU is three-way: model, host branch, device branch.
#include "arith_probe.cuh"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
using namespace zk;

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "--list") {
        for (int op = 0; op <= probe::MAX_OP_ID; op++)
            probe::dispatch(op, [&](auto tag) { using O = typename decltype(tag)::type; printf("%d %d %d %d\n", op, O::NIN, O::NOUT, O::QUAD ? 1 : 0); });
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: arith_probe_host --list | CASES OUT\n"); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open the case or the output file\n"); return 2; }
    const uint64_t bias = FpMsm<Fq377P>::hot_loop_bias();
    uint32_t head[2];
    int records = 0;
    while (fread(head, 4, 2, fi) == 2) {
        const int op = (int)head[0];
        const size_t n = head[1];
        if (n == 0 || n > probe::MAX_CASES) { fprintf(stderr, "record %d: bad case count\n", records); return 2; }
        bool ok = true;
        const bool known = probe::dispatch(op, [&](auto tag) {
            using O = typename decltype(tag)::type;
            if constexpr (O::QUAD) { fprintf(stderr, "op %d has no host body\n", op); ok = false; }
            else {
                std::vector<uint32_t> in(n * O::NIN), out(n * O::NOUT);
                if (fread(in.data(), 4, in.size(), fi) != in.size()) { fprintf(stderr, "record %d: truncated\n", records); ok = false; return; }
                for (size_t c = 0; c < n; c++) O::run(in.data() + c * O::NIN, out.data() + c * O::NOUT, bias);
                ok = fwrite(out.data(), 4, out.size(), fo) == out.size();
            }
        });
        if (!known) { fprintf(stderr, "record %d: unknown op %d\n", records, op); return 2; }
        if (!ok) return 2;
        records++;
    }
    fclose(fi);
    if (fclose(fo) != 0) return 2;
    printf("arith_probe_host ok %d\n", records);
    return 0;
}
