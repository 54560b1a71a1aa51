// ambient_plan_check.cpp -- walks demuxalot_amd/csrc/ambient_plan.h on the CPU (tests/test_ambient_cpu.py builds it with
// AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain program): every refusal of dmx_ambient_profile with its code,
// the boundaries of the grid width and of the donor rules, the order of the checks, the zero column, the count limit, and the exact
// row division for every row width a table can have.
#include <cmath>
#include <limits>

#include "ambient_plan.h"
#include "plan_check.h"

using namespace dmx::aplan;

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int G = 5;
    const long long B = 4, V = 3;
    const Facts good{true, true, false, 1, true, B, V, G};
    std::vector<float> alphas(65, 0.25f);
    const std::vector<int> d1{0, -1, 3, 4}, d2{-1, -1, 4, -1};
    const std::vector<float> soup{0.0f, 1.0f, 0.5f};
    auto status = [&](const Facts &f, long long n, const float *al, const int *a, const int *b, const float *s) { return check(f, n, al, a, b, s).status; };

    // a valid call, with and without a supplied profile
    EXPECT(status(good, 3, alphas.data(), d1.data(), d2.data(), nullptr) == OK);
    EXPECT(status(good, 3, alphas.data(), d1.data(), d2.data(), soup.data()) == OK);

    // call order, communicator
    for (int k = 0; k < 3; k++) {
        Facts f = good;
        f.have_problem = k == 1;
        f.have_table = k == 2;
        EXPECT(status(f, 3, alphas.data(), d1.data(), d2.data(), nullptr) == INVALID);
    }
    {
        Facts f = good;
        f.attached = true;
        EXPECT(status(f, 3, alphas.data(), d1.data(), d2.data(), nullptr) == UNSUPPORTED);
        f = good;
        f.nranks = 2;
        EXPECT(status(f, 3, alphas.data(), d1.data(), d2.data(), nullptr) == UNSUPPORTED);
        f = good;
        f.dense_table = false;
        EXPECT(status(f, 3, alphas.data(), d1.data(), d2.data(), nullptr) == UNSUPPORTED);
        f = good;  // no problem and a communicator: the call order is reported
        f.attached = true;
        f.have_table = false;
        EXPECT(status(f, 3, alphas.data(), d1.data(), d2.data(), nullptr) == INVALID);
    }

    // the grid's width: A = 0, 1, 64, 65 (the values behind the 64th are never read: 65 is refused before them)
    EXPECT(status(good, 0, alphas.data(), d1.data(), d2.data(), nullptr) == INVALID);
    EXPECT(status(good, -1, alphas.data(), d1.data(), d2.data(), nullptr) == INVALID);
    EXPECT(status(good, 1, alphas.data(), d1.data(), d2.data(), nullptr) == OK);
    EXPECT(status(good, 64, alphas.data(), d1.data(), d2.data(), nullptr) == OK);
    EXPECT(status(good, 65, alphas.data(), d1.data(), d2.data(), nullptr) == UNSUPPORTED);
    EXPECT(status(good, 65, nullptr, d1.data(), d2.data(), nullptr) == UNSUPPORTED);
    EXPECT(status(good, 1LL << 40, nullptr, d1.data(), d2.data(), nullptr) == UNSUPPORTED);
    EXPECT(status(good, 3, nullptr, d1.data(), d2.data(), nullptr) == INVALID);
    EXPECT(status(good, 3, alphas.data(), nullptr, d2.data(), nullptr) == INVALID);
    EXPECT(status(good, 3, alphas.data(), d1.data(), nullptr, nullptr) == INVALID);
    {
        Facts f = good;  // no barcodes: no donors to read
        f.B = 0;
        EXPECT(status(f, 3, alphas.data(), nullptr, nullptr, nullptr) == OK);
    }

    // grid values: the ends of [0, 1] are in, everything else is out - at every position of the widest grid
    for (const float ok : {0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 0.0f), std::numeric_limits<float>::denorm_min()}) {
        std::vector<float> a(64, 0.5f);
        a[63] = ok;
        EXPECT(status(good, 64, a.data(), d1.data(), d2.data(), nullptr) == OK);
    }
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -std::numeric_limits<float>::denorm_min(), 2.0f, -1.0f})
        for (int at = 0; at < 64; at++) {
            std::vector<float> a(64, 0.5f);
            a[(size_t)at] = bad;
            const Verdict verdict = check(good, 64, a.data(), d1.data(), d2.data(), nullptr);
            EXPECT(verdict.status == INVALID && verdict.at == at);
            EXPECT(status(good, at, a.data(), d1.data(), d2.data(), nullptr) == (at == 0 ? INVALID : OK));  // (a bad value behind the grid is not read)
        }

    // ambient values
    for (const float bad : {nan, inf, -inf, std::nextafter(1.0f, 2.0f), -1e-30f})
        for (long long at = 0; at < V; at++) {
            std::vector<float> s = soup;
            s[(size_t)at] = bad;
            const Verdict verdict = check(good, 3, alphas.data(), d1.data(), d2.data(), s.data());
            EXPECT(verdict.status == INVALID && verdict.at == at);
        }

    // donors: every (d1, d2) in [-3, G + 1]^2 against the rules as the header of the entry point states them
    for (int a = -3; a <= G + 1; a++)
        for (int b = -3; b <= G + 1; b++) {
            const bool skipped = a == -1, singlet = a >= 0 && a < G && b == -1, pair = a >= 0 && a < b && b < G;
            EXPECT(donors_valid(a, b, G) == (skipped || singlet || pair));
            std::vector<int> x = d1, y = d2;
            x[3] = a;
            y[3] = b;
            const Verdict verdict = check(good, 3, alphas.data(), x.data(), y.data(), nullptr);
            EXPECT(verdict.status == (skipped || singlet || pair ? OK : INVALID));
            if (verdict.status != OK) EXPECT(verdict.at == 3);
        }
    EXPECT(!donors_valid(2, 2, G));      // donor2 = donor1
    EXPECT(!donors_valid(3, 2, G));      // descending
    EXPECT(donors_valid(G - 2, G - 1, G) && !donors_valid(G - 1, G, G) && !donors_valid(G, -1, G) && !donors_valid(-2, -1, G));
    EXPECT(!donors_valid(0, -1, 0));     // no donors at all

    // the zero column: the first of several, -0 counts, none
    {
        const float a[] = {0.5f, 0.0f, 0.25f, 0.0f}, b[] = {0.5f, -0.0f}, c[] = {0.5f, 1e-45f};
        EXPECT(zero_column(4, a) == 1 && zero_column(1, a) == -1 && zero_column(2, b) == 1 && zero_column(2, c) == -1 && zero_column(0, a) == -1);
    }

    // counts: c + 1 is a float32 up to c = 2^24 - 1
    EXPECT(count_is_exact(0) && count_is_exact((1ull << 24) - 1) && !count_is_exact(1ull << 24) && !count_is_exact(~0ull));
    EXPECT((float)((1u << 24) - 1u + 1u) == 16777216.0f && (double)(float)((1u << 24) + 1u) != (double)((1u << 24) + 1u));

    // the row division: every table width up to 4096 genotypes and a few beyond, rows at both ends of the 32-bit offsets
    std::vector<unsigned> widths;
    for (unsigned g = 1; g <= 4096; g++) widths.push_back(g);
    for (unsigned g : {5000u, 65535u, 65536u, 100003u, 1u << 20, (1u << 28) - 1u, 1u << 28, (1u << 30) - 1u}) widths.push_back(g);
    for (const unsigned g : widths) {
        const unsigned row_bytes = 4u * g;
        const RowDivide d = row_divide(row_bytes);
        EXPECT((row_bytes >> d.shift) * d.inverse == 1u);
        const unsigned last = 0xFFFFFFFFu / row_bytes;  // the last row whose offset fits
        for (const unsigned row : {0u, 1u, 2u, 3u, 7u, last / 3u, last / 2u, last - (last > 0), last})
            if (row <= last) EXPECT(row_of(row * row_bytes, d.shift, d.inverse) == row);
    }

    return finish("ambient plan");
}
