"""What the entries over the resident pooled result refuse, and the layouts they derive on the host, without a GPU.

The validation is pure host code (csrc/pooled_readout_plan.h): tests/pooled_readout_plan_check.cpp walks every refusal and boundary -
the upload's pools and rows, the allowed lists, the ranges of dmx_pooled_get / _get_pool, marg_ptr, the pools' barcode lists, the slab
bounds of the option sums - built with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked into the program, and run
as a plain program (tests/check_program.py)."""
import os
import re

from tests import check_program

ROOT = check_program.ROOT
CHECKS = 134  # EXPECTs the program walks; a check that is added or lost changes the count


def test_validation_over_every_case(tmp_path):
    stdout = check_program.build_and_run(tmp_path, 'pooled_readout_plan_check')
    walked = re.search(r'pooled readout plan: (\d+) checks, 0 failures', stdout)
    assert walked and int(walked.group(1)) == CHECKS, stdout


def test_entries_are_declared_as_product_api():
    from demuxalot_amd import _lib
    debug = open(os.path.join(ROOT, 'include', 'demux_hip_debug.h')).read()
    assert re.search(r'^ \* Pooled results kept resident \(product API', debug, flags=re.M)
    for name, n_args in (('dmx_set_keep_pooled', 2), ('dmx_pooled_upload', 11), ('dmx_pooled_info', 2), ('dmx_pooled_release', 1),
                         ('dmx_pooled_get', 5), ('dmx_pooled_get_pool', 4), ('dmx_pooled_readout', 11), ('dmx_pooled_top_options', 4),
                         ('dmx_pooled_option_sums', 3), ('dmx_pooled_allowed_mass', 5)):
        assert name in _lib.DEBUG_SIGNATURES and name not in _lib.SIGNATURES
        assert len(_lib.DEBUG_SIGNATURES[name][1]) == n_args, name
    assert len(_lib.SIGNATURES) <= 64
