"""The merged weight-gradient entry points on FLOAT data, bit for bit against digests recorded on the MI355X on the commit before their
host side moved into csrc/wgrad_batch.h (``python -m tests.test_gpu_wgrad_batch_digest --record``): one table per family -- direct fp32,
Winograd, pixel-pair Winograd, bf16, fp16 -- and the SHA-256 of every ``dw``.  The integer-data tests (tests/test_gpu_conv_exact.py) give
the same sums whatever the slab boundaries and the order of the slabs; rounded fp32 sums of normal deviates do not, so a slab plan, a
workspace carving or a table order that moved shows here.  In every table the first layer is one chunk (one slab, written in place)
and others are split; the direct, half and Winograd tables launch several kernel groups (tests/test_wgrad_batch_plan_host.py reads
that from the plan text on the host).
"""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

from delora_amd import _lib
from delora_amd.models import ring_conv as rc
from tests.test_wgrad_batch_plan_host import DIGEST

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_batch_digests.json")
FAMILIES = [("direct", "f32"), ("wino", "f32"), ("pair", "f32"), ("half", "bf16"), ("half", "f16")]
ENTRY = {"direct": ("dl_conv2d_wgrad_batch_workspace_bytes", "dl_conv2d_wgrad_batch_nhwc_f32"),
         "wino": ("dl_wino_wgrad3x3_batch_workspace_bytes", "dl_wino_wgrad3x3_batch_nhwc_f32"),
         "pair": ("dl_wino_strided_wgrad3x3_batch_workspace_bytes", "dl_wino_strided_wgrad3x3_batch_nhwc_f32"),
         "half": ("dl_conv2d_wgrad_batch_h_workspace_bytes", "dl_conv2d_wgrad_batch_nhwc_h")}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPE = {"bf16": 2, "f16": 1}                         # DL_DTYPE_BF16, DL_DTYPE_F16


def digests(family, dtype, dev):
    """SHA-256 of each layer's dw [K][k][k][C] fp32 from one merged call over DIGEST[family]; workspace and dw start as NaN."""
    lib = _lib.load()
    gen = torch.Generator(device="cpu").manual_seed(20261)
    shapes = DIGEST[family]
    arr = (_lib.WgradLayer * len(shapes))()
    keep, dws = [], []
    for j, (N, H, W, C, K, ks, sh, sw) in enumerate(shapes):
        x = torch.randn((N, H, W, C), generator=gen).to(TORCH[dtype]).to(dev)
        g = torch.randn((N, rc.out_size(H, sh), rc.out_size(W, sw), K), generator=gen).to(TORCH[dtype]).to(dev)
        dw = torch.full((K, ks, ks, C), float("nan"), dtype=torch.float32, device=dev)
        keep += [x, g]
        dws.append(dw)
        arr[j].x, arr[j].g, arr[j].dw = x.data_ptr(), g.data_ptr(), dw.data_ptr()
        arr[j].N, arr[j].H, arr[j].W, arr[j].C, arr[j].K, arr[j].ksize, arr[j].stride_h, arr[j].stride_w = N, H, W, C, K, ks, sh, sw
    ap = ctypes.cast(arr, ctypes.c_void_p)
    size_fn, run_fn = ENTRY[family]
    nbytes = int(getattr(lib, size_fn)(ap, len(shapes)))
    assert nbytes > 0 and nbytes % 4 == 0, (lib.dl_last_error() or b"").decode()
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    extra = (DTYPE[dtype],) if family == "half" else ()
    _lib.check(getattr(lib, run_fn)(ap, len(shapes), ctypes.c_void_p(ws.data_ptr()), *extra,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), run_fn)
    torch.cuda.synchronize()
    out = []
    for dw in dws:
        host = dw.cpu()
        assert bool(torch.isfinite(host).all())
        out.append(hashlib.sha256(host.contiguous().numpy().tobytes()).hexdigest())
    return out


@pytest.mark.parametrize("family, dtype", FAMILIES)
def test_every_weight_gradient_of_a_merged_call_has_the_recorded_bits(family, dtype):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(GOLDEN) as f:
        recorded = json.load(f)[f"{family}-{dtype}"]
    got = digests(family, dtype, torch.device("cuda:0"))
    assert len(recorded) == len(DIGEST[family])
    differ = [(j, DIGEST[family][j]) for j, (a, b) in enumerate(zip(got, recorded)) if a != b]
    assert not differ, f"{family} {dtype}: dw differs from the recorded bits for layers {differ}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage (on the GPU): python -m tests.test_gpu_wgrad_batch_digest --record")
    dev = torch.device("cuda:0")
    rec = {f"{fam}-{dt}": digests(fam, dt, dev) for fam, dt in FAMILIES}
    again = {f"{fam}-{dt}": digests(fam, dt, dev) for fam, dt in FAMILIES}
    assert rec == again, "two runs in one process differ: the digests would record noise"
    out = os.environ.get("WGRAD_DIGEST_OUT", GOLDEN)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", out)
