"""GPU: every production sampler kernel of csrc/lm_sample.hip (the six families of fs_selftest_sample_frames, both table types, both WIDE
images) against the frame-by-frame definitions of tests/sample_refs.py: the complete sampler state after EVERY launch -- SeqState, the
penalty ring / meta / mask, the stream position or the whole SlotRng cells, the words table, XF, X, out_codes, the hidden rows, the
capture record -- exact (floats bit for bit), the prep fragments within the bound sample_refs takes from gemm_refs, every guard intact."""
import numpy as np
import pytest

import sample_refs as sr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c.name for c in sr.all_cases()])
def test_sampler_trace(name):
    case = sr.case_by_name(name)
    ref = sr.reference(case)
    got = case.run()
    assert got["L"] == case.F * case.Lf
    bad, worst = sr.compare(case, ref, got)
    print(f"{name}: {case.family}, {got['L']} launches, prep worst |err| / tol = {worst:.3f}" if case.prep else f"{name}: {case.family}, {got['L']} launches")
    assert not bad, "\n".join(bad)
    assert got["guard_ok"], "a guard around a device buffer was written"
