"""What dmx_em_doublet_shares, dmx_estep_pair_shares_resident and dmx_mstep_doublet_shares refuse, without a GPU.

The validation is a pure host function (csrc/doublet_shares_learning_plan.h: pair_shares_plan.h's check, then
doublet_learning_plan.h's check_em / check_mstep, then the share rows of the M-step): tests/doublet_shares_learning_plan_check.cpp walks
it - every refusal it borrows with its words and in its order, the share rows' own with their indices, the singlet entries that are not
read, the boundaries - built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a
plain program (tests/check_program.py)."""
import re

from tests import check_program

CHECKS = 678  # EXPECTs the program walks; a check that is added or lost changes the count


def test_validation_over_every_case(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'doublet_shares_learning_plan_check')
    walked = re.search(r'doublet shares learning plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == CHECKS, stdout
