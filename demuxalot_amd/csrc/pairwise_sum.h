// pairwise_sum.h -- np.sum of one contiguous float64 row in numpy's association, by one thread: the row sum of SNP detection's
// overall ranking (snp_detect.hip: k_sd_row_keys; snp_detection.py:223).  Plain C++ without builtins: compiled for the device by
// hipcc and for the host by any C++17 compiler (tests/pairwise_sum_check.cpp compares it with np.sum bit for bit).
//
// numpy's pairwise_sum (np.add.reduce over a contiguous row):
//   n < 8     the elements in order, starting from +0
//   n <= 128  a block: 8 interleaved partial sums r[j] (j = i mod 8) combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
//             n mod 8 leftover elements in order
//   longer    split at n / 2 rounded DOWN to a multiple of 8, left + right.  The right half is the longer one, by up to 7
//             elements more than half (rounded up), and that excess is carried down the tree: 128 << k elements are NOT always
//             down to blocks after k splits (8191 -> 4103 -> 2055 -> 1031 -> 519 -> 263 -> 135, which splits once more)
#pragma once

#if defined(__HIPCC__)
#define DMX_ROWSUM_FN __host__ __device__
#else
#define DMX_ROWSUM_FN
#endif

namespace dmx {
namespace rowsum {

constexpr int MAX_DONORS = 8192;  // the longest row (dmx_snp_count refuses more donors)
constexpr int BLOCK = 128;        // numpy's PW_BLOCKSIZE
constexpr int SPLITS = 7;         // splits the recursion below can make before it must be down to blocks

// no node that comes out of `splits` splits of n elements is longer than this (a half is at most (n + 1) / 2 + 7: monotone in n)
constexpr long long longest_after(long long n, int splits) { return splits == 0 ? n : longest_after((n + 1) / 2 + 7, splits - 1); }
static_assert(longest_after(MAX_DONORS, SPLITS) <= BLOCK, "a row of MAX_DONORS elements needs more splits than SPLITS");

template <int SPLITS_LEFT>
DMX_ROWSUM_FN inline double pairwise_sum_from(const double *a, long long n)
{
    if (n < 8) {
        double res = 0.0;
        for (long long i = 0; i < n; i++) res += a[i];
        return res;
    }
    if (SPLITS_LEFT == 0 || n <= BLOCK) {  // (SPLITS_LEFT == 0 only ends the template recursion: the static_assert keeps n <= BLOCK there)
        double r[8];
        for (int j = 0; j < 8; j++) r[j] = a[j];
        long long i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    long long n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum_from<SPLITS_LEFT ? SPLITS_LEFT - 1 : 0>(a, n2) + pairwise_sum_from<SPLITS_LEFT ? SPLITS_LEFT - 1 : 0>(a + n2, n - n2);
}

// np.sum(a[0:n]) for 0 <= n <= MAX_DONORS
DMX_ROWSUM_FN inline double pairwise_sum(const double *a, long long n) { return pairwise_sum_from<SPLITS>(a, n); }

}  // namespace rowsum
}  // namespace dmx
