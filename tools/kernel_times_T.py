"""attention / wo node times vs KV length (fs_lm_bench_kernel, bf16).  usage: kernel_times_T.py [--lib /path/libfishrt.so] [T ...]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fish-speech.rs_amd")]
args = sys.argv[1:]
if args[:1] == ["--lib"]:  # another build (a parent commit)
    from fishrt import _ffi
    _ffi.LIB_PATH = os.path.abspath(args[1]); args = args[2:]
import fishrt
from fishrt import config as fcfg
lm = fishrt.DualARTransformer(fcfg.FISH_1_5, fcfg.FISH_1_5_TOKENS, 0, "bf16").load_synthetic(0xF15E5EED)
for T in [int(a) for a in args] or (120, 250, 495, 1000, 2000, 4000, 8000):
    print(T, "attention %.2f us, wo %.2f us" % (lm.bench_kernel(1, T, 30), lm.bench_kernel(2, T, 30)))
