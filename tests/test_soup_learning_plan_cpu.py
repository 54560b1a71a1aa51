"""What dmx_mstep_soup and dmx_em_ambient_soup refuse, without a GPU.

The validation is a pure host function (csrc/soup_learning_plan.h, built on ambient_learning_plan.h's check_em and check_mstep):
tests/soup_learning_plan_check.cpp walks it - every refusal with the index it speaks of and in the words of the entries it is built on,
the order of the refusals, the boundaries of the pseudo-count, the iteration count and the unit range, and whose fraction is read - built
with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program
(tests/check_program.py)."""
import re

from tests import check_program

CHECKS = 681  # EXPECTs the program walks; a check that is added or lost changes the count


def test_validation_over_every_case(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'soup_learning_plan_check')
    walked = re.search(r'soup learning plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == CHECKS, stdout
