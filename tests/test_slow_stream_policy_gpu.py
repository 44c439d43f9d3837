"""GPU: the stream policy of the persistent slow kernel (csrc/lm_persist_slow.hip, k_slow_persist<FP8, NT>).  With NT the once-read weight
images are loaded non-temporal; no arithmetic changes, so a handle created under FISHRT_SLOW_STREAM=nt must produce the codes of a handle
created under FISHRT_SLOW_STREAM=default, element for element, on both image formats (bf16 and e4m3) -- at a prompt that crosses the 64-token
page boundary (more than one attention slice) and at a short one (a single slice, few cached tokens per slice).

What this does not show: the handle reports nothing about the instantiation it launched, so the test would also pass if the switch were ignored
and both handles ran the same kernel.  That the nt instantiation differs from the default one by the nt modifier alone is a build-time check
(DESIGN.md 4.1); that the switch selects it is what the A/B of profiles/slow_stream_policy_ab.txt measures."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import config as fcfg

SEED = 0xF15E5EED
FRAMES = 12
PROMPTS = (70, 16)
SWITCH = "FISHRT_SLOW_STREAM"


def _text_prompt(L):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(1000 + L).randint(0, fcfg.FISH_1_5_TOKENS["im_end_id"], L)
    return p


@functools.lru_cache(maxsize=None)
def _runs(dtype):
    """{(policy, L): (codes, kernels_per_frame)}: one handle per policy, one after the other (the switch is read per handle, when its
    launches are set up), both prompts on each"""
    res = {}
    saved = os.environ.get(SWITCH)
    try:
        for policy in ("default", "nt"):
            os.environ[SWITCH] = policy
            lm = fishrt.DualARTransformer(fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS, 0, dtype).load_synthetic(SEED)
            try:
                for L in PROMPTS:
                    lm.clear_slow_layer_caches()
                    out = lm.generate_blocking(_text_prompt(L), L + FRAMES - 2, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.2,
                                               seed=1, ignore_eos=True)
                    res[(policy, L)] = (out.copy(), lm.last_stats()["kernels_per_frame"])
            finally:
                lm.close()
    finally:
        if saved is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = saved
    return res


@pytest.mark.parametrize("L", PROMPTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_nt_stream_codes_equal_default_policy(dtype, L):
    r = _runs(dtype)
    (base, kpf_base), (nt, kpf_nt) = r[("default", L)], r[("nt", L)]
    assert kpf_base == 2 and kpf_nt == 2  # both ran the two persistent launches per frame, not the per-node graphs
    assert base.shape == nt.shape == (8, FRAMES)
    assert np.array_equal(base, nt)
