"""The pool arguments of the pooled entries without a GPU (dmx_estep_pools, dmx_estep_pools_resident, dmx_em_pools, dmx_estep_ambient).

What they refuse and how they lay a pool's options out are pure host functions (csrc/pools_plan.h): tests/pools_plan_check.cpp walks
them - every refusal with the index it speaks of, the order of the refusals, the 44 / 45 donor and 1024 / 1025 option boundaries,
the 16-bit column, calls without barcodes or pools, and the option words of the layout one by one - built with AddressSanitizer +
UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program (tests/check_program.py)."""
import re

from tests import check_program

CHECKS = 102  # EXPECTs the program walks; a check that is added or lost changes the count


def test_validation_and_layout_over_every_case(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'pools_plan_check')
    walked = re.search(r'pools plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == CHECKS, stdout
