"""What dmx_estep_pair_shares refuses, without a GPU.

The validation is a pure host function (csrc/pair_shares_plan.h: check - what the pooled entries refuse of the context and the pools,
then the rules of the grid of shares and of its log weights): tests/pair_shares_plan_check.cpp walks it - every refusal it borrows, met
once and ahead of the grid, and every boundary of its own rules in their order - built with AddressSanitizer +
UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_validation_over_every_case(tmp_path):
    compiler = shutil.which(os.environ.get('ASAN_CXX', 'g++'))
    assert compiler is not None, 'the pair shares plan check needs g++ (or ASAN_CXX)'
    program = str(tmp_path / 'pair_shares_plan_check')
    subprocess.check_call([compiler, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan', '-Wall', '-Wextra',
                           '-I' + os.path.join(ROOT, 'demuxalot_amd', 'csrc'), os.path.join(ROOT, 'tests', 'pair_shares_plan_check.cpp'),
                           '-o', program])
    done = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, (done.stdout[-1500:], done.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in done.stderr and 'runtime error:' not in done.stderr, done.stderr[-4000:]
    walked = re.search(r'pair shares plan: (\d+) checks, 0 failures', done.stdout)
    assert walked and int(walked.group(1)) > 500, done.stdout
