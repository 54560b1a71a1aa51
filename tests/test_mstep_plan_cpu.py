"""The M-step's policy (demuxalot_amd/csrc/mstep_plan.h: which form runs, whether it is incremental and of which kind, when the tile
records are built, where the sums go) needs no GPU: tests/mstep_plan_check.cpp includes that header alone, walks the whole cross
product of the facts the decisions read and asserts the invariants and the named rows of the decision table.
Built and run by tests/check_program.py: with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program,
as a plain program in the environment of the test run.  g++ is what `make asan` needs too: without it this test fails."""
import re

from tests import check_program


def test_mstep_plan_over_the_whole_fact_space(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'mstep_plan_check', '-O3', timeout=600)
    walked = re.search(r'mstep plan: (\d+) combinations walked, 0 failures', stdout)
    # 13 booleans and the records held or not x 3 x 3 switches x 3 genotype counts x 3 powers x 7 M-step counts x 3 horizons of the running
    # call x 2 announced horizons x 2 row counts
    assert walked and int(walked.group(1)) == 2 ** 14 * 3 * 3 * 3 * 3 * 7 * 3 * 2 * 2, stdout
