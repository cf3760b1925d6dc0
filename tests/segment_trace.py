"""Recorder of the wrapper calls ``RingSegment`` / ``RingSegmentH`` make (delora_amd/models/ring_conv.py), on the CPU and without the
library: every module-level wrapper the segments launch through is replaced by a fake that returns a zero tensor of the right shape
and dtype and appends one record -- wrapper name, arguments bound to the REAL wrapper's signature (defaults applied, so positional
versus keyword passing does not matter) and results.  Tensors are named ``t0, t1, ...`` in order of first appearance (the inputs
``x0``, ``w0..``, ``first`` beforehand), keyed by data pointer, shape, strides and dtype; every named tensor is kept alive, so no
pointer is met twice.  ``--saved--`` lists the tensors the Function kept for its backward pass, a ``--backward--`` marker separates the
passes, and the last record holds shape and strides of ``x.grad`` and of
every weight gradient.

``python -m tests.segment_trace OUT.json`` writes the traces of ``cases()``.  tests/golden/segment_traces.json was written that way by
the commit BEFORE the two segment walks became one; tests/test_segment_trace_host.py compares the present code against it."""
import inspect
import itertools
import json
import sys

import torch

from delora_amd.models import ring_conv as rc

BASE_BLOCKS = ((64, 64, (1, 1), False), (64, 128, (1, 2), True), (128, 256, (2, 2), True), (256, 256, (1, 1), False))
WRAPPERS = ("weight_storage", "conv_nhwc", "wino_conv", "wino_weights", "wino_weights_batch", "wino_strided_ok", "wino_strided_weights",
            "wino_strided_conv", "wino_strided_dgrad", "dgrad_strided", "wgrad_nhwc", "wgrad_batch", "weights_h", "weights_batch_h", "conv_nhwc_h",
            "dgrad_strided_h", "wgrad_nhwc_h", "wgrad_batch_h")


def cases():
    """{id: parameters}: the full product over precision, ``first``, ``last`` and the pixel-pair answer on the four-block segment, then
    the single cases (each in both precisions where the precision can matter)."""
    out = {}
    for half, first, last, ok in itertools.product((False, True), (True, False, "tensor"), (True, False), (True, False)):
        out[f"{'bf16' if half else 'fp32'}-first_{first}-last_{last}-pair_{ok}"] = dict(half=half, first=first, last=last, strided_ok=ok)
    for half in (False, True):
        p = "bf16" if half else "fp32"
        out[f"{p}-no_winograd"] = dict(half=half, switches={"USE_WINOGRAD": False})
        out[f"{p}-no_grad"] = dict(half=half, grad=False)
        out[f"{p}-flush_every_item"] = dict(half=half, switches={"WGRAD_PENDING_MAX_BYTES": 1})
        out[f"{p}-5x9"] = dict(half=half, hw=(5, 9), strided_ok=False)
        out[f"{p}-one_block_down"] = dict(half=half, blocks=((64, 128, (1, 2), True),))
        out[f"{p}-one_block_down_stride1"] = dict(half=half, blocks=((64, 128, (1, 1), True),))
    return out


class _Recorder:
    def __init__(self, strided_ok):
        self.records, self.names, self.keep, self.strided_ok = [], {}, [], strided_ok

    def name(self, t, name=None):
        key = (t.data_ptr(), tuple(t.shape), tuple(t.stride()), str(t.dtype))
        if key not in self.names:
            self.names[key] = name or f"t{sum(1 for n in self.names.values() if n[0] == 't')}"
            self.keep.append(t)
        return self.names[key]

    def enc(self, v):
        if torch.is_tensor(v):
            return self.name(v)
        if isinstance(v, (tuple, list)):
            return [self.enc(e) for e in v]
        if isinstance(v, torch.dtype):
            return str(v)
        assert v is None or isinstance(v, (bool, int, float, str)), type(v)
        return v

    def wrap(self, fname):
        sig, fake = inspect.signature(getattr(rc, fname)), getattr(self, "_" + fname)

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            enc_args = [self.enc(v) for v in bound.arguments.values()]       # inputs are named before the results
            result = fake(**bound.arguments)
            self.records.append([fname, enc_args, self.enc(result)])
            return result
        return call

    # -- the fakes: what the real wrapper returns, as zeros -----------------------------------------------------------
    @staticmethod
    def _weight_storage(w):
        return w.permute(0, 2, 3, 1)

    @staticmethod
    def _conv_nhwc(x, w_krsc, stride, act, epilogue, add, dsrc, transposed):
        N, H, W, _ = x.shape
        K = w_krsc.shape[3] if transposed else w_krsc.shape[0]
        return torch.zeros((N, rc.out_size(H, stride[0]), rc.out_size(W, stride[1]), K), dtype=torch.float32)

    @staticmethod
    def _wino_conv(x, u, K, act, epilogue, add, dsrc):
        return torch.zeros(tuple(x.shape[:3]) + (K,), dtype=torch.float32)

    @staticmethod
    def _u_pair(w, mul, want_fwd, want_bwd):
        n = 16 * mul * w.shape[0] * w.shape[1]
        return (torch.zeros((n,)) if want_fwd else None, torch.zeros((n,)) if want_bwd else None)

    def _wino_weights(self, w_param, want_fwd, want_bwd):
        return self._u_pair(w_param, 1, want_fwd, want_bwd)

    def _wino_weights_batch(self, w_params, want_bwd):
        return [self._u_pair(w, 1, True, want_bwd) for w in w_params]

    def _wino_strided_ok(self, N, H, W, C, K, stride):
        return self.strided_ok

    def _wino_strided_weights(self, w_param, stride, want_bwd):
        return self._u_pair(w_param, 2, True, want_bwd)

    @staticmethod
    def _wino_strided_conv(x, u_fwd, K, stride, act, epilogue):
        N, H, W, _ = x.shape
        return torch.zeros((N, H // stride[0], W // stride[1], K), dtype=torch.float32)

    @staticmethod
    def _wino_strided_dgrad(g, u_bwd, C, stride, in_hw, act, epilogue, add_grid, dsrc):
        return torch.zeros((g.shape[0], int(in_hw[0]), int(in_hw[1]), C), dtype=torch.float32)

    @staticmethod
    def _dgrad_strided(g, w_krsc, stride, in_hw, act, epilogue, add_grid, dsrc, dense):
        N, Ho, Wo, _ = g.shape
        return torch.zeros((N, Ho, Wo, w_krsc.shape[3]) if dense else (N, int(in_hw[0]), int(in_hw[1]), w_krsc.shape[3]), dtype=torch.float32)

    @staticmethod
    def _dw(x, g, ks):
        return torch.zeros((g.shape[3], ks, ks, x.shape[3]), dtype=torch.float32)

    def _wgrad_nhwc(self, x, g, ks, stride):
        return self._dw(x, g, ks)

    def _wgrad_batch(self, items):
        return [self._dw(x, g, ks) for (x, g, ks, _) in items]

    _wgrad_nhwc_h, _wgrad_batch_h = _wgrad_nhwc, _wgrad_batch

    @staticmethod
    def _w_pair_h(w, dtype, want_fwd, want_bwd):
        K, C, ks, _ = w.shape
        return (torch.zeros((ks * ks, K, C), dtype=dtype) if want_fwd else None, torch.zeros((ks * ks, C, K), dtype=dtype) if want_bwd else None)

    def _weights_h(self, w_param, dtype, want_fwd, want_bwd):
        return self._w_pair_h(w_param, dtype, want_fwd, want_bwd)

    def _weights_batch_h(self, w_params, dtype, want_bwd):
        return [self._w_pair_h(w, dtype, True, want_bwd) for w in w_params]

    @staticmethod
    def _conv_nhwc_h(x, w_prepared, ks, stride, act, epilogue, add, dsrc, transposed):
        N, H, W, _ = x.shape
        return torch.zeros((N, rc.out_size(H, stride[0]), rc.out_size(W, stride[1]), w_prepared.shape[1]), dtype=x.dtype)

    @staticmethod
    def _dgrad_strided_h(g, w_bwd, ks, stride, in_hw, act, epilogue, add_grid, dsrc, dense):
        N, Ho, Wo, _ = g.shape
        return torch.zeros((N, Ho, Wo, w_bwd.shape[1]) if dense else (N, int(in_hw[0]), int(in_hw[1]), w_bwd.shape[1]), dtype=g.dtype)


def record(half=False, first=False, last=True, strided_ok=True, grad=True, hw=(8, 64), blocks=BASE_BLOCKS, switches=None):
    """The records of one forward (+ backward) pass of the segment Function of that precision, as JSON-ready lists."""
    gen = torch.Generator().manual_seed(0)
    dtype = torch.bfloat16 if half else torch.float32
    x = torch.randn((2, hw[0], hw[1], blocks[0][0]), generator=gen).to(dtype).requires_grad_(grad)
    weights = []
    for (cin, cout, _, has_ds) in blocks:
        for shape in ((cout, cin, 3, 3), (cout, cout, 3, 3)) + (((cout, cin, 1, 1),) if has_ds else ()):
            weights.append(torch.randn(shape, generator=gen).contiguous(memory_format=torch.channels_last).requires_grad_(grad))
    if first == "tensor":
        first = torch.randn(x.shape, generator=gen).to(dtype)
    rec = _Recorder(strided_ok)
    rec.name(x, "x0")
    for i, w in enumerate(weights):
        rec.name(w, f"w{i}")
    if torch.is_tensor(first):
        rec.name(first, "first")
    saved = {n: getattr(rc, n) for n in WRAPPERS + tuple(switches or ())}
    try:
        for n in WRAPPERS:
            setattr(rc, n, rec.wrap(n))
        for n, v in (switches or {}).items():
            setattr(rc, n, v)
        y = (rc.RingSegmentH if half else rc.RingSegment).apply(x, rc.ACT["tanh"], tuple(blocks), first, last, *weights)
        rec.records.append(["--forward-result--", rec.enc(y), [list(y.shape), str(y.dtype)]])
        if grad:
            rec.records.append(["--saved--", rec.enc(list(y.grad_fn.saved_tensors))])
            rec.records.append(["--backward--"])
            y.backward(torch.zeros_like(y))
            rec.records.append(["--grads--"] + [[list(t.grad.shape), list(t.grad.stride()), str(t.grad.dtype)] for t in [x] + weights])
    finally:
        for n, v in saved.items():
            setattr(rc, n, v)
    return rec.records


def main(path):
    traces = {cid: record(**kw) for cid, kw in cases().items()}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(t, separators=(',', ':'))}" for cid, t in traces.items()) + "\n}\n")
    print(f"{len(traces)} cases, {sum(len(t) for t in traces.values())} records -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
