"""The pool arguments of the pooled entries without a GPU (dmx_estep_pools, dmx_estep_pools_resident, dmx_em_pools, dmx_estep_ambient).

What they refuse and how they lay a pool's options out are pure host functions (csrc/pools_plan.h): tests/pools_plan_check.cpp walks
them - every refusal with the index it speaks of, the order of the refusals, the 44 / 45 donor and 1024 / 1025 option boundaries,
the 16-bit column, calls without barcodes or pools, and the option words of the layout one by one - built with AddressSanitizer +
UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain program."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_validation_and_layout_over_every_case(tmp_path):
    compiler = shutil.which(os.environ.get('ASAN_CXX', 'g++'))
    assert compiler is not None, 'the pools plan check needs g++ (or ASAN_CXX)'
    program = str(tmp_path / 'pools_plan_check')
    subprocess.check_call([compiler, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan', '-Wall', '-Wextra',
                           '-I' + os.path.join(ROOT, 'demuxalot_amd', 'csrc'), os.path.join(ROOT, 'tests', 'pools_plan_check.cpp'),
                           '-o', program])
    done = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, (done.stdout[-1500:], done.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in done.stderr and 'runtime error:' not in done.stderr, done.stderr[-4000:]
    walked = re.search(r'pools plan: (\d+) checks, 0 failures', done.stdout)
    assert walked and int(walked.group(1)) > 100, done.stdout
