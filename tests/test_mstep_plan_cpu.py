"""The M-step's policy (demuxalot_amd/csrc/mstep_plan.h: which form runs, whether it is incremental and of which kind, when the tile
records are built, where the sums go) needs no GPU: tests/mstep_plan_check.cpp includes that header alone, walks the whole cross
product of the facts the decisions read and asserts the invariants and the named rows of the decision table.
Built here with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program
in the environment of the test run.  g++ is what `make asan` needs too: without it this test fails."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mstep_plan_over_the_whole_fact_space(tmp_path):
    compiler = shutil.which(os.environ.get('ASAN_CXX', 'g++'))
    assert compiler is not None, 'the policy check needs g++ (or ASAN_CXX)'
    program = str(tmp_path / 'mstep_plan_check')
    subprocess.check_call([compiler, '-std=c++17', '-O3', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan', '-Wall', '-Wextra',
                           '-I' + os.path.join(ROOT, 'demuxalot_amd', 'csrc'), os.path.join(ROOT, 'tests', 'mstep_plan_check.cpp'), '-o', program])
    done = subprocess.run([program], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, (done.stdout[-1500:], done.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in done.stderr and 'runtime error:' not in done.stderr, done.stderr[-4000:]
    walked = re.search(r'mstep plan: (\d+) combinations walked, 0 failures', done.stdout)
    # 13 booleans and the records held or not x 3 x 3 switches x 3 genotype counts x 3 powers x 7 M-step counts x 3 horizons of the running
    # call x 2 announced horizons x 2 row counts
    assert walked and int(walked.group(1)) == 2 ** 14 * 3 * 3 * 3 * 3 * 7 * 3 * 2 * 2, done.stdout
