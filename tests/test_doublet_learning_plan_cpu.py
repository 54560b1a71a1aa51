"""What dmx_em_doublets and dmx_mstep_doublets refuse, without a GPU.

The validation is a pure host function (csrc/doublet_learning_plan.h, built on pools_plan.h's check):
tests/doublet_learning_plan_check.cpp walks it - every refusal with the index it speaks of, the order of the refusals, the boundaries of
the iteration count, the power, the threshold and the unit range of the rows, and the bound of the list's length - built with
AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program
(tests/check_program.py)."""
import re

from tests import check_program

CHECKS = 615  # EXPECTs the program walks; a check that is added or lost changes the count


def test_validation_over_every_case(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'doublet_learning_plan_check')
    walked = re.search(r'doublet learning plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == CHECKS, stdout
