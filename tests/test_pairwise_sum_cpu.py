"""The float64 row sum behind SNP detection's overall ranking (demuxalot_amd/csrc/pairwise_sum.h, used by csrc/snp_detect.hip's
k_sd_row_keys) is plain C++ and needs no GPU: tests/pairwise_sum_check.cpp includes that header alone, sums the rows this test writes
and writes the sums back; they must equal np.sum of each row bit for bit.  numpy is the reference: nothing here restates how the sum is
associated.  Built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain
program (tests/check_program.py), as tests/test_mstep_plan_cpu.py does.  Without g++ (or ASAN_CXX) this test fails."""
import numpy as np

from tests import check_program
from tests import fixture_io as fio

# every leaf and the first splits, and every length around the ones whose halves stay above 128 elements after six splits (7689..8191)
LENGTHS = list(range(1, 301)) + list(range(7600, 8193))


def test_row_sum_equals_numpy_bit_for_bit(tmp_path):
    rng = np.random.default_rng(20)
    rows = [np.square(rng.uniform(-1., 1., n)) for n in LENGTHS]  # squares of uniform numbers, as the importances are
    with open(tmp_path / 'rows.bin', 'wb') as f:
        f.write(np.int64(len(rows)).tobytes())
        for row in rows:
            f.write(np.int64(len(row)).tobytes())
            f.write(row.astype('<f8').tobytes())
    stdout = check_program.build_and_run(tmp_path, 'pairwise_sum_check', '-O3', ['-ffp-contract=off'],
                                         [tmp_path / 'rows.bin', tmp_path / 'sums.bin'], timeout=600)
    assert f'pairwise sum: {len(rows)} rows' in stdout
    sums = np.fromfile(tmp_path / 'sums.bin', dtype='<f8')
    want = np.array([np.sum(row) for row in rows])
    assert sums.shape == want.shape
    differ = [n for n, a, b in zip(LENGTHS, sums, want) if a.tobytes() != b.tobytes()]
    assert not differ, f'{len(differ)} row lengths whose sum differs from np.sum: {differ[:20]}'
    fio.assert_bitwise(sums, want, 'row sums')
