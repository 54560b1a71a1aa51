"""The context's validity flags (csrc/ctx_state.h: CtxState), without a GPU.

tests/ctx_state_check.cpp walks every transition from many states (the flags it names take the stated values, every other flag keeps
its own), replays three call sequences as the host code composes them, and checks the invariants of DESIGN.md 4.15 over seeded random
sequences - built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run as a plain
program.  The source test reads demuxalot_amd/csrc: no file but ctx_state.h assigns a flag."""
import glob
import os
import re

from tests import check_program

CSRC = check_program.CSRC

# Fields of OTHER structs that share a flag's name: (file, object, field).  estep_plan.h's Facts copies two flags for the plan to read
# (estep_facts), kernels.h's EstepArgs carries the floor the kernels build the codes with (fill_estep_args).
OTHER_STRUCTS = {('dmx_steps.cpp', 'f', 'prob16_valid'), ('dmx_steps.cpp', 'f', 'dict_candidate'), ('dmx_steps.cpp', 'a', 'nz_floor')}


def header_flags():
    """The data members of CtxState, read from the header: everything declared with an initialiser ahead of the first member function."""
    text = open(os.path.join(CSRC, 'ctx_state.h')).read()
    body = text[text.index('struct CtxState {'):]
    members = body[:body.index('void ')]
    flags = re.findall(r'^\s+(?:bool|float|int|long long)\s+(\w+)\s*=\s*[^;]+;', members, flags=re.M)
    assert len(flags) == len(set(flags)) and len(flags) >= 18, flags
    return flags


def without_comments_and_strings(text):
    text = re.sub(r'/\*.*?\*/', lambda m: re.sub(r'[^\n]', ' ', m.group()), text, flags=re.S)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r'//[^\n]*', '', text)


def test_transitions_sequences_and_invariants(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'ctx_state_check')
    walked = re.search(r'ctx state: (\d+) flags compared, (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(2)) > 100_000, stdout
    assert int(walked.group(1)) == len(header_flags()), 'a flag of ctx_state.h that the walker does not compare'


def test_only_ctx_state_h_assigns_a_flag():
    flags = '|'.join(header_flags())
    assign = r'\s*(?:=(?!=)|\+\+|--|[-+*/%|&^]=|<<=|>>=)'
    through_object = re.compile(r'([\w\]\)]+)\s*(?:->|\.)\s*(' + flags + r')\b' + assign)
    increment_ahead = re.compile(r'(?:\+\+|--)\s*[\w\]\)]+\s*(?:->|\.)\s*(' + flags + r')\b')
    bare = re.compile(r'(?:^|[;{}(),])\s*(' + flags + r')\b' + assign, flags=re.M)  # (a member function of a struct that derives from CtxState)
    found = []
    sources = sorted(p for ext in ('cpp', 'hip', 'h') for p in glob.glob(os.path.join(CSRC, '*.' + ext)))
    assert len(sources) > 40 and os.path.join(CSRC, 'ctx_state.h') in sources
    for path in sources:
        name = os.path.basename(path)
        if name == 'ctx_state.h':
            continue
        text = without_comments_and_strings(open(path).read())
        for number, line in enumerate(text.split('\n'), 1):
            for m in through_object.finditer(line):
                if (name, m.group(1), m.group(2)) not in OTHER_STRUCTS:
                    found.append(f'{name}:{number}: {line.strip()}')
            if increment_ahead.search(line) or bare.search(line):
                found.append(f'{name}:{number}: {line.strip()}')
    assert not found, 'flags of CtxState assigned outside ctx_state.h (add a transition there):\n' + '\n'.join(found)
    # the search does find what it is for: the transitions themselves
    own = without_comments_and_strings(open(os.path.join(CSRC, 'ctx_state.h')).read())
    assert len(bare.findall(own)) >= 40
    assert through_object.search('    c->incr_valid = false;') and through_object.search('ctx.nz_rebuilds++;') and not through_object.search('if (c->incr_valid == x)')
