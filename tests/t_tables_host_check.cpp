// tests/t_tables_host_check.cpp -- build_t_tables (csrc/marlin_host.hpp), the builder of the column-bucketed tables behind round 2's t, checked on the host under
// -fsanitize=address,undefined by tests/test_r1cs_model.py.  A stand-alone program: nothing of it is loaded into python.
//   t_tables_host_check <cases file>      (written by tests/r1cs_cases.py write_cases: the matrices of the t cases of tests/test_gpu_r1cs.py)
// For every case: every entry of A, B, C appears exactly once, in the bucket of its re-indexed column; every segment is non-empty, at most T_SEG long and the segments of a
// column tile its bucket in order; col_seg_ptr is monotone from 0 to nseg; the heavy list is exactly the columns above the threshold, ascending; the arrays the device
// reads are never empty.  Prints "case <i> <nseg> <n_heavy> <largest segment count>" per case and "t_tables_host_check ok" at the end.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>
#include "marlin_host.hpp"

using namespace zk;
using namespace zk::hostx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "case %zu: check failed at line %d: %s\n", g_case, __LINE__, #c); exit(1); } } while (0)
static size_t g_case = 0;

template <class T> static std::vector<T> take(FILE *f, size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "short cases file\n"); exit(2); }
    return v;
}
static uint64_t take64(FILE *f) { return take<uint64_t>(f, 1)[0]; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: t_tables_host_check <cases file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const size_t ncases = take64(f);
    for (g_case = 0; g_case < ncases; g_case++) {
        const size_t n = take64(f), m = take64(f), rows = take64(f);
        const uint32_t t_seg = (uint32_t)take64(f), t_heavy = (uint32_t)take64(f);
        CsrMatrix M[3];
        size_t total = 0;
        for (int q = 0; q < 3; q++) {
            const size_t nnz = take64(f);
            M[q].rowptr = take<uint32_t>(f, rows + 1); M[q].col = take<uint32_t>(f, nnz); M[q].coeff = take<int64_t>(f, nnz);
            CHECK(M[q].rowptr[rows] == nnz);
            total += nnz;
        }
        const TTables T = build_t_tables(n, m, rows, M[0], M[1], M[2], t_seg, t_heavy);
        // the buckets: every entry exactly once, under its re-indexed column
        CHECK(T.colptr.size() == n + 1 && T.colptr[0] == 0 && T.colptr[n] == total);
        CHECK(T.trow.size() == std::max<size_t>(total, 1) && T.tmat.size() == T.trow.size() && T.tcoef.size() == T.trow.size());
        typedef std::tuple<uint32_t, uint32_t, uint8_t, int64_t> Entry;       // (bucket, row, matrix, coefficient)
        std::vector<Entry> want, got;
        for (int q = 0; q < 3; q++)
            for (size_t r = 0; r < rows; r++)
                for (uint32_t i = M[q].rowptr[r]; i < M[q].rowptr[r + 1]; i++) want.emplace_back((uint32_t)reindex_by_subdomain(n, m, M[q].col[i]), (uint32_t)r, (uint8_t)q, M[q].coeff[i]);
        for (size_t h = 0; h < n; h++) {
            CHECK(T.colptr[h] <= T.colptr[h + 1]);
            for (uint32_t e = T.colptr[h]; e < T.colptr[h + 1]; e++) { CHECK(T.trow[e] < rows && T.tmat[e] < 3); got.emplace_back((uint32_t)h, T.trow[e], T.tmat[e], T.tcoef[e]); }
        }
        std::sort(want.begin(), want.end()); std::sort(got.begin(), got.end());
        CHECK(want.size() == total && got == want);
        // the segments
        CHECK(T.col_seg_ptr.size() == n + 1 && T.col_seg_ptr[0] == 0 && T.col_seg_ptr[n] == T.nseg);
        CHECK(T.seg_start.size() == std::max<size_t>(T.nseg, 1) && T.seg_end.size() == T.seg_start.size());
        uint32_t widest = 0;
        std::vector<uint32_t> heavy;
        for (size_t h = 0; h < n; h++) {
            CHECK(T.col_seg_ptr[h] <= T.col_seg_ptr[h + 1]);
            uint32_t at = T.colptr[h];
            for (uint32_t sg = T.col_seg_ptr[h]; sg < T.col_seg_ptr[h + 1]; sg++) {
                CHECK(T.seg_start[sg] == at && T.seg_end[sg] > T.seg_start[sg] && T.seg_end[sg] - T.seg_start[sg] <= t_seg && T.seg_end[sg] <= T.colptr[h + 1]);
                CHECK(T.seg_end[sg] - T.seg_start[sg] == t_seg || sg + 1 == T.col_seg_ptr[h + 1]);      // only a column's last segment is short
                at = T.seg_end[sg];
            }
            CHECK(at == T.colptr[h + 1]);
            const uint32_t segs = T.col_seg_ptr[h + 1] - T.col_seg_ptr[h];
            widest = std::max(widest, segs);
            if (segs > t_heavy) heavy.push_back((uint32_t)h);
        }
        // the heavy list
        CHECK(T.n_heavy == heavy.size());
        if (heavy.empty()) CHECK(T.heavy.size() == 1 && T.heavy[0] < n);      // the dummy that keeps the device array non-empty names a real column
        else CHECK(T.heavy == heavy);
        printf("case %zu %u %u %u\n", g_case, T.nseg, T.n_heavy, widest);
    }
    uint8_t extra;
    if (fread(&extra, 1, 1, f) != 0) { fprintf(stderr, "trailing bytes in the cases file\n"); return 2; }
    fclose(f);
    printf("t_tables_host_check ok\n");
    return 0;
}
