"""The E-step's policy (demuxalot_amd/csrc/estep_plan.h: which arithmetic runs, whether the dictionary or the packed form takes the
E-step, what a guarded E-step builds, releases and converts, what its fine level walks, which kernel a launch is) needs no GPU:
tests/estep_plan_check.cpp includes that header alone, replays run_estep's sequence of the plan's stages over the cross product of
the facts the decisions interact on (the others cycle along the walk) and asserts the invariants and the named rows of the decision table.
Built and run by tests/check_program.py: with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program,
as a plain program in the environment of the test run.  g++ is what `make asan` needs too: without it this test fails."""
import re

from tests import check_program


def test_estep_plan_over_the_whole_fact_space(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'estep_plan_check', '-O3', timeout=600)
    walked = re.search(r'estep plan: (\d+) combinations walked, 0 failures', stdout)
    # 36 option tables (18 singlet widths on either side of every routing threshold, 18 doublet tables up to K = 8256) x 3 modes x prior or
    # not x logits kept or not x 2 barcode counts x 3 table heights x (3 schedule switches x bins or none) x (tile stream, coarse records:
    # there or not) x (3 coarse-pass switches x adaptive or not x lean memory or not x 2 clips) x 7 states of the dictionary's switch,
    # candidate and row array x record size x 7 states of the packing switch and the long-row statistic.  The five facts that feed one
    # predicate each (binary16 table valid, sliced, table lists, split rows, pair blocks) cycle through their 32 states along the walk, and the
    # dictionary build's 6 results behind them: they do not multiply it, so this is the cross product of the facts above, not of all.
    assert walked and int(walked.group(1)) == 36 * 3 * 2 * 2 * 2 * 3 * (3 * 2) * (2 * 2) * (3 * 2 * 2 * 2) * 7 * 2 * 7, stdout
