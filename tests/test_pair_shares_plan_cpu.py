"""What dmx_estep_pair_shares refuses, without a GPU.

The validation is a pure host function (csrc/pair_shares_plan.h: check - what the pooled entries refuse of the context and the pools,
then the rules of the grid of shares and of its log weights): tests/pair_shares_plan_check.cpp walks it - every refusal it borrows, met
once and ahead of the grid, and every boundary of its own rules in their order - built with AddressSanitizer +
UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program (tests/check_program.py)."""
import re

from tests import check_program

CHECKS = 831  # EXPECTs the program walks; a check that is added or lost changes the count


def test_validation_over_every_case(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'pair_shares_plan_check')
    walked = re.search(r'pair shares plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == CHECKS, stdout
