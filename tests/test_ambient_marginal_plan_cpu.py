"""What dmx_estep_ambient_grid_marginal refuses, without a GPU.

The validation is a pure host function (csrc/ambient_grid_plan.h: check_marginal - the max entry's check and the rule of the log
weights): tests/ambient_marginal_plan_check.cpp walks it - every refusal it borrows, met once and ahead of the weights, and every
boundary of the weights' rule - built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and
run as a plain program (tests/check_program.py)."""
import re

from tests import check_program

CHECKS = 417  # EXPECTs the program walks; a check that is added or lost changes the count


def test_validation_over_every_case(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'ambient_marginal_plan_check')
    walked = re.search(r'ambient marginal plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == CHECKS, stdout
