"""What dmx_em_doublet_shares, dmx_estep_pair_shares_resident and dmx_mstep_doublet_shares refuse, without a GPU.

The validation is a pure host function (csrc/doublet_shares_learning_plan.h: pair_shares_plan.h's check, then
doublet_learning_plan.h's check_em / check_mstep, then the share rows of the M-step): tests/doublet_shares_learning_plan_check.cpp walks
it - every refusal it borrows with its words and in its order, the share rows' own with their indices, the singlet entries that are not
read, the boundaries - built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a
plain program."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_validation_over_every_case(tmp_path):
    compiler = shutil.which(os.environ.get('ASAN_CXX', 'g++'))
    assert compiler is not None, 'the doublet shares learning plan check needs g++ (or ASAN_CXX)'
    program = str(tmp_path / 'doublet_shares_learning_plan_check')
    subprocess.check_call([compiler, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan', '-Wall', '-Wextra',
                           '-I' + os.path.join(ROOT, 'demuxalot_amd', 'csrc'), os.path.join(ROOT, 'tests', 'doublet_shares_learning_plan_check.cpp'),
                           '-o', program])
    done = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, (done.stdout[-1500:], done.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in done.stderr and 'runtime error:' not in done.stderr, done.stderr[-4000:]
    walked = re.search(r'doublet shares learning plan: (\d+) checks, 0 failures', done.stdout)
    assert walked and int(walked.group(1)) > 500, done.stdout
