"""CPU: budgets of the half-sum filter scan (fscan_mx_kernel_cascade), read from the built library and its ISA: no scratch, one
1024-thread block per CU (<= 128 VGPRs: four waves per SIMD), and no instruction touching a register with a load in flight."""
import pytest

from tests.test_isa_invariants import _tool, asm_path  # noqa: F401  (module fixture)
from tests.test_kernel_resources import resources, waves_per_simd  # noqa: F401  (module fixture)

NAME = "_ZN6riiamd23fscan_mx_kernel_cascadeENS_6FsArgsE"


def test_cascade_scan_budget(resources):
    assert NAME in resources, "kernel renamed? " + NAME
    d = resources[NAME]
    assert int(d["private_segment_fixed_size"]) == 0 and int(d["vgpr_spill_count"]) == 0, d
    assert waves_per_simd(d) >= 4, d


def test_cascade_scan_isa_inflight_clean(asm_path):
    t = _tool()
    funcs = t.split_functions(asm_path)
    assert NAME in funcs
    probs, ninst = t.check_function(NAME, funcs[NAME])
    assert ninst > 100
    assert not probs, probs[:3]
