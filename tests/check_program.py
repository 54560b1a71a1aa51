"""The check programs of the pure host headers (tests/*_check.cpp) are built and run in one way: with AddressSanitizer +
UndefinedBehaviorSanitizer, their runtimes linked into the program, as a plain program under a time limit.  Without g++ (or ASAN_CXX)
the calling test fails."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'demuxalot_amd', 'csrc')


def build_and_run(tmp_path, name, level='-O1', flags=(), args=(), timeout=300):
    """Builds tests/<name>.cpp into tmp_path and runs it with `args`: it must exit 0 and neither sanitizer may report anything.
    Returns the program's stdout; what it says there is the calling test's to judge."""
    compiler = shutil.which(os.environ.get('ASAN_CXX', 'g++'))
    assert compiler is not None, f'{name} needs g++ (or ASAN_CXX)'
    program = str(tmp_path / name)
    subprocess.check_call([compiler, '-std=c++17', level, '-g', *flags, '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan', '-Wall', '-Wextra', '-I' + CSRC,
                           os.path.join(ROOT, 'tests', name + '.cpp'), '-o', program])
    done = subprocess.run([program, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    assert done.returncode == 0, (done.stdout[-1500:], done.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in done.stderr and 'runtime error:' not in done.stderr, done.stderr[-4000:]
    return done.stdout
