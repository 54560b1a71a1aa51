"""What dmx_em_ambient, dmx_mstep_ambient and dmx_estep_ambient_resident refuse, without a GPU.

The validation is a pure host function (csrc/ambient_learning_plan.h, built on ambient_scoring_plan.h's check):
tests/ambient_learning_plan_check.cpp walks it - every refusal with the index it speaks of, the order of the refusals, the boundaries of
the iteration count, the power and the unit range, and whose fraction is read - built with AddressSanitizer +
UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program (tests/check_program.py)."""
import re

from tests import check_program

CHECKS = 293  # EXPECTs the program walks; a check that is added or lost changes the count


def test_validation_over_every_case(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'ambient_learning_plan_check')
    walked = re.search(r'ambient learning plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == CHECKS, stdout
