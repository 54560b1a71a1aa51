// The float64 row sum of SNP detection's overall ranking (demuxalot_amd/csrc/pairwise_sum.h) on the host: reads rows of float64 from a
// file, writes one sum per row.  tests/test_pairwise_sum_cpu.py writes the rows and compares the sums with np.sum bit for bit; nothing
// here knows how the sum is associated.
//
//   pairwise_sum_check <rows> <sums>
//   rows: int64 row count, then per row an int64 length n (0 <= n <= MAX_DONORS) and n float64 values
//   sums: one float64 per row
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pairwise_sum.h"

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <rows> <sums>\n", argv[0]);
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb");
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    int64_t n_rows = 0;
    if (std::fread(&n_rows, sizeof n_rows, 1, in) != 1 || n_rows < 0) return 3;
    for (int64_t r = 0; r < n_rows; r++) {
        int64_t n = 0;
        if (std::fread(&n, sizeof n, 1, in) != 1 || n < 0 || n > dmx::rowsum::MAX_DONORS) return 3;
        std::vector<double> row((size_t)n);  // an allocation of exactly n: a read past the row's end is AddressSanitizer's to report
        if (n && std::fread(row.data(), sizeof(double), (size_t)n, in) != (size_t)n) return 3;
        const double sum = dmx::rowsum::pairwise_sum(row.data(), n);
        if (std::fwrite(&sum, sizeof sum, 1, out) != 1) return 4;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 4;
    std::printf("pairwise sum: %lld rows\n", (long long)n_rows);
    return 0;
}
