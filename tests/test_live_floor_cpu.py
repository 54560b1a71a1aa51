"""The live floor of the fixed-point M-step forms needs no GPU: tests/live_floor_check.cpp includes csrc/kernels.h (the floors, and through
fixed_point.h the very conversion the kernels add with) and csrc/mstep_plan.h, walks the plan asked ahead of an M-step (sums_on_grid) against
the form launch() then yields over the fact space, and runs every float32 posterior in [2^-27, 2^-25] x 5 keep factors x shifts 0 .. 50 through
fixed_of: at or below the floor the added integer is 0.  Built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into
the program, and run as a plain program (tests/check_program.py, as tests/test_mstep_plan_cpu.py does)."""
import os
import re

from tests import check_program


def test_live_floor_plan_and_proof(tmp_path):
    flags = ['-pthread', '-D__HIP_PLATFORM_AMD__', '-I' + os.path.join(check_program.ROOT, 'include'), '-I/opt/rocm/include']
    stdout = check_program.build_and_run(tmp_path, 'live_floor_check', '-O3', flags, timeout=600)
    said = re.search(r'live floor: (\d+) plan combinations walked, (\d+) conversions tried, first non-zero posterior (\S+) \(floor (\S+)\), 0 failures',
                     stdout)
    assert said, stdout
    # 12 booleans x 3 x 3 switches x 3 genotype counts x 3 powers x 7 M-step counts x 3 horizons x 2 announced horizons
    assert int(said.group(1)) == 2 ** 12 * 3 * 3 * 3 * 3 * 7 * 3 * 2
    # every float32 of two binades (and 2^-25 itself) x 5 keep factors x 51 shifts
    assert int(said.group(2)) == (2 * 2 ** 23 + 1) * 5 * 51
    # the codes' rule: live <=> p >= 2^-26; the first posterior that adds anything at keep 1, shift 50 is sqrt(2) x 2^-26, rounded up
    assert float.fromhex(said.group(4)) == 2.0 ** -26 * (1 - 2.0 ** -24)
    assert 2.0 ** -26 < float.fromhex(said.group(3)) < 2.0 ** -25
