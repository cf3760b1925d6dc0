"""Channels-last convolutions of the pose CNN on the fp32 matrix cores: thin torch wrappers over ``dl_conv2d_nhwc_f32`` /
``dl_conv2d_wgrad_nhwc_f32`` (include/delora_hip.h) and the autograd Function of the whole residual trunk.

Reference: ``ResNetModified._forward_impl`` / ``BasicBlock.forward`` (src/models/resnet_modified.py:95-120, :159-177) --
17 x (F.pad circular + Conv2d) + tanh + residual adds under torch autograd.  Here the trunk (layer1..layer4) is ONE
autograd Function on channels-last activations ``[N,H,W,C]``:

  forward   per block   y1 = act(conv(x, w1));  y2 = act(conv(y1, w2) + shortcut)       2 (+1) launches, nothing else
  backward  per block   dW2 = wgrad(y1, g2);  g1 = dgrad(g2, w2) * act'(y1);  dW1 = wgrad(x, g1);
                        g2_prev = (dgrad(g1, w1) + g2) * act'(x)                         4 (+2) launches, nothing else

where g denotes a gradient with respect to a PRE-activation: the activation derivative of the previous block and the
shortcut gradient are folded into the epilogue of the input-gradient convolution, so no elementwise kernel runs between
two convolutions.  The wrap-around of the image width and the zero rows above / below are addressing inside the kernels:
no padded copy of an activation exists.  Weights are the torch parameters themselves in channels_last memory format
(``[K][3][3][C]`` storage); weight gradients are written in the same layout.

The strided layers' input gradients run one pass per stride phase with exactly the taps whose phase matches
(``dgrad_strided``); no library convolution is left in the trunk.
"""
import ctypes
import os

import torch

from .. import _lib

ACT = {"none": 0, "tanh": 1, "relu": 2}
USE_WINOGRAD = True          # stride-1 3x3 layers as fused Winograd F(2x2,3x3) (csrc/wino.hip); False: the direct kernel
EPI_ADD, EPI_ACT, EPI_DACT, EPI_ADD_GRID = 1, 2, 4, 8


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Base-address skew of the activation tensors this module allocates (bytes, cycled per allocation; 0 = off).  Tensors that one
# kernel streams together (x, y, shortcut, saved activation) otherwise start at addresses a large power of two apart.
ALLOC_SKEW = 0
_skew_state = {"i": 0}


def _empty(shape, dtype, device):
    if not ALLOC_SKEW:
        return torch.empty(shape, dtype=dtype, device=device)
    n = 1
    for d in shape:
        n *= int(d)
    esz = torch.empty((), dtype=dtype).element_size()
    _skew_state["i"] = (_skew_state["i"] + 1) % 8
    off = (_skew_state["i"] * ALLOC_SKEW) // esz
    return torch.empty((n + (8 * ALLOC_SKEW) // esz,), dtype=dtype, device=device)[off:off + n].view(shape)


def weight_storage(w):
    """The parameter ``[K,C,k,k]`` viewed as its channels_last storage ``[K,k,k,C]`` (no copy when it already has that
    memory format -- ``OdometryModel`` converts its convolution weights once)."""
    v = w.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def grad_for(dw_krsc, w_param):
    """The weight gradient ``dW [K,k,k,C]`` as the gradient tensor of the parameter ``[K,C,k,k]`` (or of its ``(shape, stride)``
    pair): the same memory, with the parameter's own strides.  For a 1x1 filter the permuted view has strides (C,1,C,C) while the
    parameter keeps (C,1,1,1) -- the same layout, but DistributedDataParallel compares strides literally and would copy the
    gradient into its bucket view on every step ("Grad strides do not match bucket view strides")."""
    shape, stride = (tuple(w_param.shape), tuple(w_param.stride())) if torch.is_tensor(w_param) else w_param
    g = dw_krsc.permute(0, 3, 1, 2)
    if tuple(g.stride()) != stride and shape[2] == 1 and shape[3] == 1 and stride[0] == shape[1] and stride[1] == 1:
        g = g.as_strided(shape, stride)
    return g


def out_size(n, stride):
    """Output extent of the reference's padded convolutions (3x3 with one pad pixel per side -- circular on the width, zeros on the
    height -- or 1x1 unpadded; src/models/resnet_modified.py:97-102, :159-177): floor((n - 1) / stride) + 1 = ceil(n / stride)."""
    return -(-int(n) // int(stride))


def conv_nhwc(x, w_krsc, stride=(1, 1), act=0, epilogue=0, add=None, dsrc=None, transposed=False):
    """``y = epilogue(conv(x, w))`` on channels-last fp32 tensors.  x ``[N,H,W,C]``; w ``[K,k,k,C]`` (``transposed``: the
    forward weight ``[C,k,k,K]`` of the layer whose input gradient is computed, x then being the output gradient)."""
    lib = _lib.load()
    N, H, W, C = x.shape
    ks = w_krsc.shape[1]
    K = w_krsc.shape[3] if transposed else w_krsc.shape[0]
    y = _empty((N, out_size(H, stride[0]), out_size(W, stride[1]), K), torch.float32, x.device)
    _lib.check(lib.dl_conv2d_nhwc_f32(_ptr(x), _ptr(w_krsc), _ptr(y), _ptr(add), _ptr(dsrc), N, H, W, C, K, ks, stride[0],
                                      stride[1], int(transposed), int(act), int(epilogue), _stream()), "dl_conv2d_nhwc_f32")
    return y


USE_WINOGRAD_WGRAD = True    # stride-1 3x3 weight gradients with >= 128 input channels in the Winograd domain (csrc/wino.hip)


def wgrad_nhwc(x, g, ks, stride=(1, 1)):
    """``dW [K,k,k,C]`` (channels_last storage of the parameter gradient) from input x ``[N,H,W,C]`` and output gradient g.
    Stride-1 3x3 layers with at least 128 input channels take the Winograd-domain kernel (6-9 % faster there; the 64-channel
    layers and everything strided stay on the direct kernel)."""
    lib = _lib.load()
    N, H, W, C = x.shape
    K = g.shape[3]
    dw = torch.empty((K, ks, ks, C), dtype=torch.float32, device=x.device)
    if USE_WINOGRAD_WGRAD and ks == 3 and tuple(stride) == (1, 1) and C >= 128:
        nbytes = lib.dl_wino_wgrad_workspace_bytes(N, H, W, C, K)
        if nbytes:
            ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
            _lib.check(lib.dl_wino_wgrad3x3_nhwc_f32(_ptr(x), _ptr(g), _ptr(dw), _ptr(ws), N, H, W, C, K, _stream()),
                       "dl_wino_wgrad3x3_nhwc_f32")
            return dw
    ws = torch.empty((lib.dl_conv2d_wgrad_workspace_bytes(N, H, W, C, K, ks, stride[0], stride[1]) // 4,), dtype=torch.float32,
                     device=x.device)
    _lib.check(lib.dl_conv2d_wgrad_nhwc_f32(_ptr(x), _ptr(g), _ptr(dw), _ptr(ws), N, H, W, C, K, ks, stride[0], stride[1],
                                            _stream()), "dl_conv2d_wgrad_nhwc_f32")
    return dw


def _wgrad_layer_table(part):
    """ctypes table of ``dl_wgrad_layer`` for (x, g, ks, stride) items + the freshly allocated fp32 ``dW [K,k,k,C]`` of each."""
    arr = (_lib.WgradLayer * len(part))()
    dws = []
    for j, (x, g, ks, stride) in enumerate(part):
        N, H, W, C = x.shape
        K = g.shape[3]
        dw = torch.empty((K, ks, ks, C), dtype=torch.float32, device=x.device)
        dws.append(dw)
        arr[j].x, arr[j].g, arr[j].dw = x.data_ptr(), g.data_ptr(), dw.data_ptr()
        arr[j].N, arr[j].H, arr[j].W, arr[j].C, arr[j].K = N, H, W, C, K
        arr[j].ksize, arr[j].stride_h, arr[j].stride_w = ks, stride[0], stride[1]
    return arr, dws


def _wgrad_batch_call(items, size_fn, run_fn, what, *extra):
    lib = _lib.load()
    out = []
    for i0 in range(0, len(items), _lib.WGRAD_BATCH):
        part = items[i0:i0 + _lib.WGRAD_BATCH]
        arr, dws = _wgrad_layer_table(part)
        ap = ctypes.cast(arr, ctypes.c_void_p)
        nbytes = getattr(lib, size_fn)(ap, len(part))
        if not nbytes:
            raise _lib.DeloraHipError(what + ": " + (lib.dl_last_error() or b"").decode())
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=part[0][0].device)
        _lib.check(getattr(lib, run_fn)(ap, len(part), _ptr(ws), *extra, _stream()), what)
        out += dws
    return out


USE_WINOGRAD_STRIDED_WGRAD = True    # stride-(1,2) 3x3 weight gradients on the pixel-pair view, live planes only (honoured only with USE_WINOGRAD)
# Dispatch policy on top of the shape rule: chunks of 8 tiles the pair view has per output block.  Below one chunk per CU a block's slabs
# cannot fill the chip and every workgroup is prologue and plane stores only; nothing that small was measured, so it stays direct.
WINO_STRIDED_WGRAD_MIN_CHUNKS = 256


def wino_strided_wgrad_ok(N, H, W, C, K, stride):
    """The shape rule of ``dl_wino_strided_wgrad_takes``, restated (no library call per layer and step): stride (1,2), even H, W a multiple
    of 32, C and K multiples of 64, the pair view ``[N,H,W/2,2C]`` / ``[N,H,W/2,K]`` within the 32-bit offsets of the kernel."""
    if tuple(stride) != (1, 2) or min(N, H, W, C, K) <= 0 or H % 2 or W % 32 or C % 64 or K % 64:
        return False
    wide = max(2 * C, K)
    return N * H * (W // 2) * wide < 2 ** 31 and H * (W // 2) * wide < 2 ** 30


def wgrad_batch(items):
    """The fp32 weight gradients of several layers in merged launches (include/delora_hip.h: ``dl_wgrad_layer``): ``items`` = list of
    (x, g, ks, stride); returns ``dW [K,k,k,C]`` per item.  Stride-1 3x3 layers with at least 128 input channels take the Winograd-domain
    kernel (as ``wgrad_nhwc`` decides), stride-(1,2) 3x3 layers that ``wino_strided_wgrad_ok`` takes and that are large enough the
    pixel-pair form of it (``USE_WINOGRAD_STRIDED_WGRAD``), the rest the direct one; within each family the layers that share a kernel run in ONE launch
    with far fewer pixel slabs (fp32 partial copies of the gradient) per layer than a launch of their own needs.  A narrow network's layers
    (fewer than 64 channels on a side) are not merged: each takes the narrow family's launch pair (``narrow_wgrad``)."""
    wino, strided, direct = [], [], []
    out = [None] * len(items)
    for i, (x, g, ks, stride) in enumerate(items):
        N, H, W, C = x.shape
        K = g.shape[3]
        if C % 64 or K % 64:                           # a narrow network's layer: a launch pair of its own (csrc/narrow.hip)
            out[i] = narrow_wgrad(x, g, ks, stride)
            continue
        # (the shape rule of dl_wino_wgrad_workspace_bytes, restated here: one library call per layer and step is host time)
        if (USE_WINOGRAD_WGRAD and ks == 3 and tuple(stride) == (1, 1) and C >= WINO_WGRAD_MIN_C_BATCHED and C % 64 == 0 and K % 64 == 0 and W >= 2
                and N * H * W * max(C, K) < 2 ** 31 and H * W * max(C, K) < 2 ** 30):
            wino.append(i)
        elif (USE_WINOGRAD and USE_WINOGRAD_STRIDED_WGRAD and ks == 3 and wino_strided_wgrad_ok(N, H, W, C, K, stride)
                and N * (H // 2) * (W // 32) >= WINO_STRIDED_WGRAD_MIN_CHUNKS):
            strided.append(i)
        else:
            direct.append(i)
    if strided:
        for i, dw in zip(strided, _wgrad_batch_call([items[i] for i in strided], "dl_wino_strided_wgrad3x3_batch_workspace_bytes",
                                                    "dl_wino_strided_wgrad3x3_batch_nhwc_f32", "dl_wino_strided_wgrad3x3_batch_nhwc_f32")):
            out[i] = dw
    if wino:
        for i, dw in zip(wino, _wgrad_batch_call([items[i] for i in wino], "dl_wino_wgrad3x3_batch_workspace_bytes", "dl_wino_wgrad3x3_batch_nhwc_f32",
                                                 "dl_wino_wgrad3x3_batch_nhwc_f32")):
            out[i] = dw
    if direct:
        for i, dw in zip(direct, _wgrad_batch_call([items[i] for i in direct], "dl_conv2d_wgrad_batch_workspace_bytes", "dl_conv2d_wgrad_batch_nhwc_f32",
                                                   "dl_conv2d_wgrad_batch_nhwc_f32")):
            out[i] = dw
    return out


def wino_ok(H, W, C, K):
    """Whether the fused Winograd F(2x2,3x3) kernel (csrc/wino.hip) takes a stride-1 3x3 layer of this shape: any image size (groups
    of 64 tiles hang over the edge of images that do not divide; odd sizes end in partial tiles), channel counts that tile."""
    return H >= 1 and W >= 1 and C % 8 == 0 and K % 64 == 0


def wino_weights(w_param, want_fwd=True, want_bwd=True):
    """Winograd-domain weights of a 3x3 layer: (u_fwd, u_bwd: 16 K C floats each in the blocked layout of csrc/wino.hip: wn_u_index) from the parameter ``[K,C,3,3]``."""
    lib = _lib.load()
    w = weight_storage(w_param)
    K, C = w.shape[0], w.shape[3]
    n = lib.dl_wino_weights_floats(K, C)
    uf = torch.empty((n,), dtype=torch.float32, device=w.device) if want_fwd else None
    ub = torch.empty((n,), dtype=torch.float32, device=w.device) if want_bwd else None
    _lib.check(lib.dl_wino_weights_f32(_ptr(w), _ptr(uf), _ptr(ub), K, C, _stream()), "dl_wino_weights_f32")
    return uf, ub


def wino_weights_batch(w_params, want_bwd=True):
    """Winograd-domain weights of several 3x3 layers in ONE launch (``dl_wino_weights_batch_f32``): a list of (u_fwd, u_bwd) in the
    order of ``w_params``; the outputs of all layers are views of two allocations."""
    lib = _lib.load()
    ws = [weight_storage(w) for w in w_params]
    out = []
    if not ws:
        return out
    sizes = [int(lib.dl_wino_weights_floats(w.shape[0], w.shape[3])) for w in ws]
    dev = ws[0].device
    uf_all = torch.empty((sum(sizes),), dtype=torch.float32, device=dev)
    ub_all = torch.empty((sum(sizes),), dtype=torch.float32, device=dev) if want_bwd else None
    off = 0
    for n in sizes:
        out.append((uf_all[off:off + n], ub_all[off:off + n] if want_bwd else None))
        off += n
    for i0 in range(0, len(ws), _lib.WINO_BATCH):
        part = list(range(i0, min(i0 + _lib.WINO_BATCH, len(ws))))
        arr = (_lib.WinoLayer * len(part))()
        for j, i in enumerate(part):
            arr[j].w = ws[i].data_ptr()
            arr[j].u_fwd = out[i][0].data_ptr()
            arr[j].u_bwd = out[i][1].data_ptr() if want_bwd else None
            arr[j].K, arr[j].C = ws[i].shape[0], ws[i].shape[3]
        _lib.check(lib.dl_wino_weights_batch_f32(ctypes.cast(arr, ctypes.c_void_p), len(part), _stream()), "dl_wino_weights_batch_f32")
    return out


def wino_conv(x, u, K, act=0, epilogue=0, add=None, dsrc=None):
    """Stride-1 3x3 convolution of x ``[N,H,W,C]`` with Winograd-domain weights ``u`` (u_fwd: forward; u_bwd with the
    output gradient as x: input gradient) -> ``[N,H,W,K]``, epilogue as conv_nhwc."""
    lib = _lib.load()
    N, H, W, C = x.shape
    y = _empty((N, H, W, K), torch.float32, x.device)
    # a launch with few tile groups (batch 1) splits its input channels over otherwise idle CUs and needs scratch for the partial sums
    key = (N, H, W, C, K)
    nbytes = _WINO_WS_BYTES.get(key)
    if nbytes is None:
        nbytes = _WINO_WS_BYTES[key] = int(lib.dl_wino_conv3x3_workspace_bytes(N, H, W, C, K))
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device) if nbytes else None
    _lib.check(lib.dl_wino_conv3x3_nhwc_f32(_ptr(x), _ptr(u), _ptr(y), _ptr(add), _ptr(dsrc), N, H, W, C, K, int(act),
                                            int(epilogue), _ptr(ws), _stream()), "dl_wino_conv3x3_nhwc_f32")
    return y


_WINO_WS_BYTES = {}

USE_WINOGRAD_STRIDED = True  # stride-(1,2) 3x3 layers on the Winograd kernel through the pixel-pair view (honoured only with USE_WINOGRAD)
STRIDED_PLAN_CUS = 0         # CU count the plan query is asked with (0: the device's own)
_STRIDED_TAKES = {}


def wino_strided_ok(N, H, W, C, K, stride):
    """Whether the dispatch runs a strided 3x3 layer (input ``[N,H,W,C]``) as pixel-pair Winograd: ``dl_wino_strided_takes``."""
    key = (N, H, W, C, K, tuple(stride), STRIDED_PLAN_CUS)
    ok = _STRIDED_TAKES.get(key)
    if ok is None:
        ok = _STRIDED_TAKES[key] = bool(_lib.load().dl_wino_strided_takes(N, H, W, C, K, stride[0], stride[1], STRIDED_PLAN_CUS))
    return ok


def wino_strided_weights(w_param, stride, want_bwd=True):
    """(u_fwd, u_bwd) of a strided 3x3 layer's rearranged kernel (csrc/wino.hip: k_wino_weights_strided) from the parameter ``[K,C,3,3]``."""
    lib = _lib.load()
    w = weight_storage(w_param)
    K, C = w.shape[0], w.shape[3]
    n = int(lib.dl_wino_strided_weights_floats(K, C, stride[0], stride[1]))
    uf = torch.empty((n,), dtype=torch.float32, device=w.device)
    ub = torch.empty((n,), dtype=torch.float32, device=w.device) if want_bwd else None
    _lib.check(lib.dl_wino_strided_weights_f32(_ptr(w), _ptr(uf), _ptr(ub), K, C, stride[0], stride[1], _stream()), "dl_wino_strided_weights_f32")
    return uf, ub


def wino_strided_conv(x, u_fwd, K, stride, act=0, epilogue=0):
    """Strided 3x3 convolution of x ``[N,H,W,C]`` with the weights of ``wino_strided_weights`` -> ``[N,H/sh,W/sw,K]``."""
    N, H, W, C = x.shape
    y = _empty((N, H // stride[0], W // stride[1], K), torch.float32, x.device)
    _lib.check(_lib.load().dl_wino_strided_conv3x3_nhwc_f32(_ptr(x), _ptr(u_fwd), _ptr(y), N, H, W, C, K, stride[0], stride[1], int(act),
                                                           int(epilogue), _stream()), "dl_wino_strided_conv3x3_nhwc_f32")
    return y


def wino_strided_dgrad(g, u_bwd, C, stride, in_hw, act=0, epilogue=0, add_grid=None, dsrc=None):
    """Input gradient ``[N,H,W,C]`` of the same layer from g ``[N,H/sh,W/sw,K]``; epilogue as ``dgrad_strided``."""
    N, Ho, Wo, K = g.shape
    H, W = int(in_hw[0]), int(in_hw[1])
    assert Ho * stride[0] == H and Wo * stride[1] == W, (g.shape, in_hw, stride)
    dx = _empty((N, H, W, C), torch.float32, g.device)
    _lib.check(_lib.load().dl_wino_strided_dgrad3x3_nhwc_f32(_ptr(g), _ptr(u_bwd), _ptr(dx), _ptr(add_grid), _ptr(dsrc), N, H, W, K, C, stride[0],
                                                            stride[1], int(act), int(epilogue), _stream()), "dl_wino_strided_dgrad3x3_nhwc_f32")
    return dx


def supported(x_shape, blocks, narrow=False):
    """Whether the fp32 HIP trunk can run these shapes: channel counts multiples of 64, or, with ``narrow`` -- the first layers of a narrow
    network (``factor_fewer_resnet_channels`` 2 and 4), asked for by the 8-channel pose network alone -- multiples of 16 inside the narrow
    family's domain at stride (1,1) / (1,2).  The image size is free: tiles hang over the edge
    of feature maps that do not divide, odd widths / heights included -- the reference's shipped 64x720 image (feature maps 180, 90,
    45 and 23 pixels wide, config/config_datasets.yaml:21) and 64x512 (layer4: 32x16, :47) run here like BASELINE's 64x2048."""
    return _supported(x_shape, blocks, 1 << 31, narrow=narrow)


def _channels_tile(c, narrow):
    return c % 64 == 0 or (narrow and c % 16 == 0 and narrow_ok(c, c))


def _supported(x_shape, blocks, max_elements, narrow=False):
    """``max_elements``: the C side indexes a tensor with 32-bit element (fp32) / byte (half) offsets and rejects N*H*W*max(C,K) at or
    above 2^31 (conv.hip, wino.hip) resp. 2^30 (convh.hip, wgradh.hip); the Winograd kernels additionally keep a sample's H*W*C below
    2^30.  The same bounds here let cnn_impl 'auto' fall back to the module path instead of raising from the C side.  ``narrow``: 16,
    32 and 48 channels count as well (fp32 only: csrc/narrow.hip), at the strides that family has."""
    N, H, W, C = x_shape
    if not _channels_tile(C, narrow) or H < 1 or W < 1:
        return False
    for (cin, cout, stride, _) in blocks:
        if (not _channels_tile(cin, narrow) or not _channels_tile(cout, narrow) or stride[0] not in (1, 2) or stride[1] not in (1, 2)
                or (stride[0] == 2 and stride[1] == 1)):
            return False
        if (cin % 64 or cout % 64) and (stride[0] != 1 or not narrow_ok(cin, cout)):
            return False
        wide = max(cin, cout, 64 if (cin % 64 or cout % 64) else 0)         # (the narrow family bounds N*H*W*64)
        if N * H * W * wide >= max_elements or H * W * wide >= (1 << 30):
            return False
        H, W = out_size(H, stride[0]), out_size(W, stride[1])
    return True


def _seam_workspace(N, H, W, C, ks, stride, dense, device):
    """fp32 ``[N,H,2,C]`` scratch for the two seam terms of a stride-2-in-width 3x3 layer on an ODD image width (the stride phases do
    not close under the wrap-around there; csrc/conv.hip: k_dgrad_oddw_seam), else None."""
    if ks == 3 and stride[1] == 2 and W % 2 == 1 and W >= 3 and not dense:
        return torch.empty((N, H, 2, C), dtype=torch.float32, device=device)
    return None


def dgrad_strided(g, w_krsc, stride, in_hw, act=0, epilogue=0, add_grid=None, dsrc=None, dense=False):
    """Input gradient of a strided layer whose INPUT image is ``in_hw`` = (H, W): g ``[N,Ho,Wo,K]`` (Ho = ceil(H / sh), Wo = ceil(W /
    sw)) with the layer's forward weight ``[K,k,k,C]`` -> ``[N,H,W,C]`` (``dense``: the 1x1 layers' gradient kept on the grid
    ``[N,Ho,Wo,C]``)."""
    lib = _lib.load()
    N, Ho, Wo, K = g.shape
    H, W = int(in_hw[0]), int(in_hw[1])
    assert Ho == out_size(H, stride[0]) and Wo == out_size(W, stride[1]), (g.shape, in_hw, stride)
    ks, C = w_krsc.shape[1], w_krsc.shape[3]
    shape = (N, Ho, Wo, C) if dense else (N, H, W, C)
    dx = _empty(shape, torch.float32, g.device)
    seam = _seam_workspace(N, H, W, C, ks, stride, dense, g.device)
    _lib.check(lib.dl_conv2d_dgrad_strided_nhwc_f32(_ptr(g), _ptr(w_krsc), _ptr(dx), _ptr(add_grid), _ptr(dsrc), N, H, W, K, C, ks,
                                                    stride[0], stride[1], int(dense), int(act), int(epilogue), _ptr(seam), _stream()),
               "dl_conv2d_dgrad_strided_nhwc_f32")
    return dx


def pool_fwd(a):
    """Stem max-pooling (3x3, stride (1,2), wrap-around width) of a ``[N,H,W,C]`` -> (y ``[N,H,W/2,C]``, win int8)."""
    lib = _lib.load()
    N, H, W, C = a.shape
    y = torch.empty((N, H, W // 2, C), dtype=torch.float32, device=a.device)
    win = torch.empty((N, H, W // 2, C), dtype=torch.int8, device=a.device)
    _lib.check(lib.dl_pool3x3s12_nhwc_fwd(_ptr(a), N, H, W, C, _ptr(y), _ptr(win), _stream()), "dl_pool3x3s12_nhwc_fwd")
    return y, win


def pool_bwd(g, a, win, act):
    """Gradient of ``pool_fwd(act(.))`` with respect to the PRE-activation conv1 output: ``[N,H,W,C]``."""
    lib = _lib.load()
    N, H, W, C = a.shape
    out = torch.empty_like(a)
    _lib.check(lib.dl_pool3x3s12_nhwc_bwd(_ptr(g), _ptr(a), _ptr(win), N, H, W, C, int(act), _ptr(out), _stream()),
               "dl_pool3x3s12_nhwc_bwd")
    return out


class MeanHW(torch.autograd.Function):
    """Global average pooling of a channels-last map ``[N,H,W,C]`` -> ``[N,C]`` (avgpool + flatten of the reference) as one
    deterministic kernel; the backward is the broadcast of ``g / (H*W)``."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = x.contiguous()
        N, H, W, C = x.shape
        y = torch.empty((N, C), dtype=torch.float32, device=x.device)
        _lib.check(lib.dl_mean_hw_nhwc_f32(_ptr(x), N, H * W, C, _ptr(y), _stream()), "dl_mean_hw_nhwc_f32")
        ctx.shape = (N, H, W, C)
        return y

    @staticmethod
    def backward(ctx, g):
        N, H, W, C = ctx.shape
        return (g * (1.0 / (H * W))).view(N, 1, 1, C).expand(N, H, W, C)


# ---------------------------------------------------------------------------------------------------------------------
# Dropout on the HIP path (csrc/dropout.hip; the stream's contract is in include/delora_hip.h).  The three sites of the reference
# (src/models/resnet_modified.py:95-118): the stacked input (inside the stem's transposing copy), the channels of layer3's output
# (``ChannelDropout`` between two trunk segments) and the fc output (inside the fused heads).
SITE_INPUT, SITE_CHANNELS, SITE_FC = 1, 2, 3
_SEED_MIX = 0x9E3779B97F4A7C15


def draw_seed(device):
    """One 64-bit seed for the three sites of a forward pass, drawn ON THE DEVICE by torch's generator: ``torch.manual_seed`` governs
    it, and a captured graph draws a fresh one on every replay (torch registers its generator with the capture)."""
    return torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, device=device)


def mix_rank(seed, rank, world_size):
    """The seed of one rank of several: ranks seeded alike must not drop alike.  A device-side xor with a constant of the rank
    (splitmix64's finaliser of rank + 1); a single process keeps the seed as drawn."""
    if world_size <= 1:
        return seed
    z = ((int(rank) + 1) * _SEED_MIX) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    z ^= z >> 31
    return seed ^ (z - 2 ** 64 if z >= 2 ** 63 else z)


def dropout_scale(seed, site, p, n):
    """``scale [n]`` fp32 = 0 or 1 / (1 - p) for the n decisions of a site (``dl_dropout_scale_f32``); seed = int64 device tensor."""
    lib = _lib.load()
    scale = torch.empty((int(n),), dtype=torch.float32, device=seed.device)
    _lib.check(lib.dl_dropout_scale_f32(_ptr(seed), int(site), float(p), int(n), _ptr(scale), _stream()), "dl_dropout_scale_f32")
    return scale


def stem_input_drop(x, seed, p):
    """Planar ``[N,C,H,W]`` fp32 -> channels-last ``[N,H,W,C]`` with the site-1 dropout applied on the way (one launch)."""
    lib = _lib.load()
    x = x.contiguous()
    N, C, H, W = x.shape
    x8 = torch.empty((N, H, W, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.dl_stem_input_nhwc_drop_f32(_ptr(x), N, C, H, W, _ptr(seed), float(p), _ptr(x8), _stream()), "dl_stem_input_nhwc_drop_f32")
    return x8


_DTYPE_CODE_ANY = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}         # DL_DTYPE_F32 / _F16 / _BF16


class ChannelDropout(torch.autograd.Function):
    """``y = x * scale[n][c]`` on a channels-last map between two trunk segments (Dropout2d of the reference,
    src/models/resnet_modified.py:112), fp32 / fp16 / bf16.  It sits at a cut of the trunk, where gradients travel in the segments'
    private convention, and serves either arrangement:
      * ``act = 0`` (what ``_run_segments`` uses): the segment behind it is handed the UN-dropped x as the source of its activation
        derivative (``first`` = that tensor), so the gradient arriving here already carries ``act'(x)`` and the backward is
        ``g * scale`` -- exact for scale 0 and 1, hence bit-identical to the uncut trunk when nothing is dropped;
      * ``act != 0``: behind a segment run with ``first=True`` it RECEIVES a true ``dL/dy`` and RETURNS ``g * scale * act'(x)`` in one
        pass (``dl_channel_scale_bwd_act_nhwc_t``) from the saved un-dropped x.  In half precision the true ``dL/dy`` is one more stored
        -- rounded -- tensor than the uncut trunk has: measured 6e-3 (bf16) / 7e-4 (fp16) of conv1's weight gradient at p = 0, which
        is why the trunk does not use this arrangement."""

    @staticmethod
    def forward(ctx, x, scale, act):
        x = x.contiguous()
        ctx.save_for_backward(*((x, scale) if act else (scale,)))
        ctx.act = int(act)
        return channel_scale(x, scale)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        if not ctx.act:
            (scale,) = ctx.saved_tensors
            g_pre = channel_scale(g, scale)
        else:
            lib = _lib.load()
            x, scale = ctx.saved_tensors
            N, H, W, C = x.shape
            g_pre = torch.empty_like(x)
            _lib.check(lib.dl_channel_scale_bwd_act_nhwc_t(_ptr(g), _ptr(x), _ptr(scale), N, H * W, C, ctx.act, _DTYPE_CODE_ANY[x.dtype], _ptr(g_pre),
                                                           _stream()), "dl_channel_scale_bwd_act_nhwc_t")
        if BACKWARD_TRACE is not None:
            BACKWARD_TRACE.append(("channel_dropout", g.shape[3]))
        return g_pre, None, None


def channel_scale(x, scale):
    """``x [N,H,W,C] * scale [N,C]`` (``dl_channel_scale_nhwc_t``; fp32 arithmetic, one rounding to x's type)."""
    lib = _lib.load()
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    _lib.check(lib.dl_channel_scale_nhwc_t(_ptr(x), _ptr(scale), N, H * W, C, _DTYPE_CODE_ANY[x.dtype], _ptr(y), _stream()), "dl_channel_scale_nhwc_t")
    return y


TOWER_CHANNELS = 80          # stem input behind the per-image feature tower: 2 x 40 channels
TOWER_PITCH = 128            # ... held in a [N,H,W,128] buffer whose channels 80..127 are zero (``RingStemWide``)
NARROW_STEM_CHANNELS = (16, 32)      # conv1 outputs of factor_fewer_resnet_channels 4 and 2 (factor 8 stays on the module path)


def stem_supported(x_shape, out_channels):
    """Whether the HIP stem takes an input ``[N,C,H,W]``: ``RingStem`` for 8 input channels per chunk, ``RingStemWide`` for the 80
    channels of the feature tower; 64-channel output tiles -- or, for the 8-channel planar stem alone, the 16 / 32 output channels of a
    narrow network (conv1 on csrc/narrow.hip) --, a width that halves twice."""
    N, C, H, W = x_shape
    k_ok = out_channels % 64 == 0 or (C == 8 and out_channels in NARROW_STEM_CHANNELS and N * H * W * 64 < (1 << 31))
    return ((C % 8 == 0 and C % 16 != 0) or C == TOWER_CHANNELS) and k_ok and W % 4 == 0 and W >= 4 and H >= 1


def planar_stem_supported(x_shape, out_channels):
    """``stem_supported`` for the planar-input ``RingStem`` alone (its fused weight gradient is the 8-channel network's path)."""
    return stem_supported(x_shape, out_channels) and x_shape[1] % 16 != 0


class RingStem(torch.autograd.Function):
    """conv1 (3x3, stride (1,2), wrap-around width) + activation + the 3x3 / stride (1,2) max-pooling of the stem on
    channels-last tensors (reference resnet_modified.py:97-102): ``[N,8,H,W]`` planar input -> ``[N,H,W/4,64]``.  Forward:
    one transposing copy of the 8-channel input, the direct MFMA convolution with the activation in its epilogue, the
    pooling kernel.  Backward: pooling backward + activation derivative + conv1's weight gradient in ONE kernel
    (``dl_stem_wgrad_f32``); only when the gradient with respect to the INPUT image is wanted (never in training: the range image
    is data) the three steps run separately with the library's convolution backward.  A narrow network's conv1 (16 / 32 output
    channels) runs on the narrow family (``narrow_conv``); its backward is the pooling backward + the strided ``narrow_wgrad``, two
    launches and a slab sum instead of the fused kernel, which stays the 64-channel path.  The 134 MB pre-pooling map is kept for
    the backward (the pooled output is not: the trunk saves it).

    An optional fourth argument ``drop = (seed, p)`` applies the element-wise input dropout (site 1 of csrc/dropout.hip) inside the
    transposing copy (``dl_stem_input_nhwc_drop_f32``); the dropped channels-last image is what the backward's weight gradient reads.
    No mask is stored: the gradient with respect to the input image regenerates it from the saved seed."""

    @staticmethod
    def forward(ctx, x, w1, act, *drop):
        if drop and drop[0] is not None:
            seed, p = drop[0]
            x8 = stem_input_drop(x, seed, p)
            ctx.drop_p = float(p)
        else:
            seed = None
            x8 = x.permute(0, 2, 3, 1).contiguous()
        ctx.n_extra = len(drop)
        conv1 = conv_nhwc if w1.shape[0] % 64 == 0 else narrow_conv          # (a narrow network's 16 / 32 output channels)
        a = conv1(x8, weight_storage(w1), stride=(1, 2), act=act, epilogue=EPI_ACT if act else 0)
        y, win = pool_fwd(a)
        ctx.save_for_backward(x8, a, win, w1, *([seed] if seed is not None else []))
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, g):
        x8, a, win, w1, *seed = ctx.saved_tensors
        extra = (None,) * ctx.n_extra
        want_x = ctx.needs_input_grad[0]
        lib = _lib.load()
        N, H, W, _ = x8.shape
        nbytes = 0 if want_x or a.shape[3] != 64 or x8.shape[3] != 8 else lib.dl_stem_wgrad_workspace_bytes(N, H, W)
        if nbytes:
            # the usual case (the range image is data): pooling backward + act' + conv1's weight gradient in ONE kernel, the
            # gradient with respect to conv1's pre-activation (134 MB at batch 8) is never written (csrc/stem.hip: k_stem_wgrad)
            ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x8.device)
            dw = torch.empty((64, 8, 3, 3), dtype=torch.float32, device=x8.device)
            _lib.check(lib.dl_stem_wgrad_f32(_ptr(g.contiguous()), _ptr(a), _ptr(win), _ptr(x8), N, H, W, int(ctx.act), _ptr(ws), _ptr(dw),
                                             _stream()), "dl_stem_wgrad_f32")
            return (None, dw, None) + extra
        gc = pool_bwd(g.contiguous(), a, win, ctx.act)
        if not want_x and a.shape[3] % 64:
            # a narrow network's conv1: the strided weight gradient of the narrow family, laid out as the parameter is
            dw = narrow_wgrad(x8, gc, 3, stride=(1, 2)).permute(0, 3, 1, 2)
            return (None, dw if tuple(dw.stride()) == tuple(w1.stride()) else dw.contiguous(), None) + extra
        xp = torch.cat((x8[:, :, -1:], x8, x8[:, :, :1]), dim=2).permute(0, 3, 1, 2)       # wrapped, channels_last strides
        gx, dw, _ = torch.ops.aten.convolution_backward(gc.permute(0, 3, 1, 2), xp, w1, None, (1, 2), (1, 0), (1, 1), False,
                                                        (0, 0), 1, (want_x, True, False))
        if want_x:                                     # fold the two wrap columns back
            gxp = gx
            gx = gxp[..., 1:-1].clone()
            gx[..., -1] += gxp[..., 0]
            gx[..., 0] += gxp[..., -1]
            if seed:                                   # the input went through the dropout: the same mask, from the saved seed
                gx = gx * dropout_scale(seed[0], SITE_INPUT, ctx.drop_p, x8.numel()).view(x8.shape).permute(0, 3, 1, 2)
        return ((gx if want_x else None), dw, None) + extra


# ---------------------------------------------------------------------------------------------------------------------
# The per-image feature tower of ``pre_feature_extraction`` (reference src/models/model.py:30-54) on the narrow family
# (csrc/tower.hip) and the 80-channel stem behind it.
TOWER_PLAN = ((4, 8), (8, 16), (16, 24), (24, 32), (32, 40))         # (C, K) of the five layers


def _view(pitch, offset=0, group=1):
    """{pitch, offset, group} of include/delora_hip.h (narrow family): a dense ``[N,H,W,CH]`` tensor is ``_view(CH)``."""
    return (ctypes.c_int32 * 3)(int(pitch), int(offset), int(group))


def tower_conv(x, w, y, shape, x_view, y_view, act=0, epilogue=0, dsrc=None, dsrc_view=None, transposed=False):
    """``y = epilogue(conv(x, w))`` of the narrow family into the caller's ``y``: ``shape`` = (N, H, W, C, K); w ``[K,3,3,C]``
    (``transposed``: the forward weight ``[C,3,3,K]`` of the layer whose input gradient is taken); views as ``_view``."""
    lib = _lib.load()
    N, H, W, C, K = shape
    _lib.check(lib.dl_tower_conv3x3_nhwc_f32(_ptr(x), _ptr(w), _ptr(y), _ptr(dsrc), N, H, W, C, K, x_view, y_view, dsrc_view, int(transposed),
                                             int(act), int(epilogue), _stream()), "dl_tower_conv3x3_nhwc_f32")
    return y


def tower_wgrad(x, g, shape, x_view, g_view):
    """``dW [K,3,3,C]`` of a narrow layer from its input x and output gradient g (views as ``_view``); fixed-order partial sums."""
    lib = _lib.load()
    N, H, W, C, K = shape
    nbytes = lib.dl_tower_wgrad_workspace_bytes(N, H, W, C, K)
    if not nbytes:
        raise _lib.DeloraHipError(f"dl_tower_wgrad3x3_nhwc_f32 does not support N={N} H={H} W={W} C={C} K={K}")
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
    dw = torch.empty((K, 3, 3, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.dl_tower_wgrad3x3_nhwc_f32(_ptr(x), _ptr(g), _ptr(dw), _ptr(ws), N, H, W, C, K, x_view, g_view, _stream()),
               "dl_tower_wgrad3x3_nhwc_f32")
    return dw


def tower_supported(x_shape):
    """Whether ``RingTower`` takes a planar input ``[B,8,H,W]``: two 4-channel images per sample, a wide stem input below 2^31
    elements (the C side's 32-bit offsets)."""
    B, C, H, W = x_shape
    return C == 8 and B >= 1 and H >= 1 and W >= 1 and B * H * W * TOWER_PITCH < (1 << 31)


# ---------------------------------------------------------------------------------------------------------------------
# Narrow pose networks (``factor_fewer_resnet_channels`` 2 and 4): the layers whose channel counts are not multiples of 64 on the narrow
# family's strided / 1x1 / residual members (csrc/narrow.hip).
def narrow_ok(cin, cout):
    """The channel domain of the narrow family (csrc/narrow.hip: nr_channels_ok), restated."""
    return 4 <= cin <= 64 and 8 <= cout <= 64 and cin % 4 == 0 and cout % 8 == 0


def narrow_conv(x, w_krsc, stride=(1, 1), act=0, epilogue=0, add=None, dsrc=None, transposed=False):
    """``conv_nhwc`` on the narrow family (``dl_narrow_conv2d_nhwc_f32``): same arguments, 4..64 channels, stride (1,1) or (1,2)."""
    lib = _lib.load()
    N, H, W, C = x.shape
    ks = w_krsc.shape[1]
    K = w_krsc.shape[3] if transposed else w_krsc.shape[0]
    y = _empty((N, out_size(H, stride[0]), out_size(W, stride[1]), K), torch.float32, x.device)
    _lib.check(lib.dl_narrow_conv2d_nhwc_f32(_ptr(x), _ptr(w_krsc), _ptr(y), _ptr(add), _ptr(dsrc), N, H, W, C, K, ks, stride[0], stride[1],
                                             int(transposed), int(act), int(epilogue), _stream()), "dl_narrow_conv2d_nhwc_f32")
    return y


def narrow_dgrad_strided(g, w_krsc, stride, in_hw, act=0, epilogue=0, add_grid=None, dsrc=None, dense=False):
    """``dgrad_strided`` on the narrow family (``dl_narrow_dgrad_strided_nhwc_f32``): the output gradient read with zeros between its
    columns, as addressing."""
    lib = _lib.load()
    N, Ho, Wo, K = g.shape
    H, W = int(in_hw[0]), int(in_hw[1])
    assert Ho == out_size(H, stride[0]) and Wo == out_size(W, stride[1]), (g.shape, in_hw, stride)
    ks, C = w_krsc.shape[1], w_krsc.shape[3]
    dx = _empty((N, Ho, Wo, C) if dense else (N, H, W, C), torch.float32, g.device)
    _lib.check(lib.dl_narrow_dgrad_strided_nhwc_f32(_ptr(g), _ptr(w_krsc), _ptr(dx), _ptr(add_grid), _ptr(dsrc), N, H, W, K, C, ks, stride[0],
                                                    stride[1], int(dense), int(act), int(epilogue), _stream()), "dl_narrow_dgrad_strided_nhwc_f32")
    return dx


def narrow_wgrad(x, g, ks, stride=(1, 1)):
    """``wgrad_nhwc`` on the narrow family (``dl_narrow_wgrad_nhwc_f32``): fixed-order partial sums, a launch pair per layer."""
    lib = _lib.load()
    N, H, W, C = x.shape
    K = g.shape[3]
    nbytes = lib.dl_narrow_wgrad_workspace_bytes(N, H, W, C, K, ks, stride[0], stride[1])
    if not nbytes:
        raise _lib.DeloraHipError(f"dl_narrow_wgrad_nhwc_f32 does not support x {tuple(x.shape)} -> K={K}, kernel {ks}, stride {tuple(stride)}")
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
    dw = torch.empty((K, ks, ks, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.dl_narrow_wgrad_nhwc_f32(_ptr(x), _ptr(g), _ptr(dw), _ptr(ws), N, H, W, C, K, ks, stride[0], stride[1], _stream()),
               "dl_narrow_wgrad_nhwc_f32")
    return dw


def _tower_backward(g, gv, acts, weights, act, N, H, W):
    """Layers 5..1 of the tower's backward from ``g`` = the gradient of layer 5's PRE-activation, laid out as the view ``gv``: per
    layer the weight gradient, then the input gradient with act' of the layer below in its epilogue.  Returns the five weight
    gradients in the parameters' layout."""
    grads = [None] * 5
    for i in range(4, -1, -1):
        C, K = TOWER_PLAN[i]
        grads[i] = grad_for(tower_wgrad(acts[i], g, (N, H, W, C, K), _view(C), gv), weights[i])
        if i:
            gp = _empty((N, H, W, C), torch.float32, g.device)
            tower_conv(g, weight_storage(weights[i]), gp, (N, H, W, K, C), gv, _view(C), act=act, epilogue=EPI_DACT if act else 0,
                       dsrc=acts[i] if act else None, dsrc_view=_view(C) if act else None, transposed=True)
            g, gv = gp, _view(C)
    return grads


class RingTower(torch.autograd.Function):
    """The five 3x3 ring convolutions + activation in front of the pose CNN (reference src/models/model.py:30-54), for both images
    of every sample at once: planar ``[B,8,H,W]`` (= ``[2B,4,H,W]``) + the five weights -> the channels-last stem input
    ``[B,H,W,128]`` whose channels 0..39 / 40..79 hold the towers of image 1 / image 2 and whose channels 80..127 are zero
    (``RingStemWide`` reads it as a 128-channel input of the direct kernels).  One transposing copy makes ``[2B,H,W,4]``; every
    layer is ONE launch over 2B images; the fifth writes both slices of the wide buffer through its view, so the reference's
    ``torch.cat`` is never a copy.  The five activations are kept for the backward (act' and weight-gradient inputs).

    Backward: layers 5..1; the act' of layer i-1 sits in the epilogue of layer i's input gradient.  ``last``: the incoming gradient
    is a true ``dL/dy`` and act' of the output is applied here; ``RingStemWide`` hands over the gradient of the PRE-activation
    (the private convention of ``RingSegment``) and passes ``last = False``.  The image is data: no gradient is returned for it."""

    @staticmethod
    def forward(ctx, x, act, last, *weights):
        B, _, H, W = x.shape
        N = 2 * B
        a = x.contiguous().view(N, 4, H, W).permute(0, 2, 3, 1).contiguous()
        acts = [a]
        ws = [weight_storage(w) for w in weights]
        for i, (C, K) in enumerate(TOWER_PLAN):
            if i < 4:
                y, yv = _empty((N, H, W, K), torch.float32, x.device), _view(K)
            else:
                y, yv = _empty((B, H, W, TOWER_PITCH), torch.float32, x.device), _view(TOWER_PITCH, 0, 2)
                y[..., TOWER_CHANNELS:].zero_()
            tower_conv(a, ws[i], y, (N, H, W, C, K), _view(C), yv, act=act, epilogue=EPI_ACT if act else 0)
            acts.append(y)
            a = y
        ctx.save_for_backward(*acts, *weights)
        ctx.act, ctx.last = act, bool(last)
        return a

    @staticmethod
    def backward(ctx, gy):
        saved = ctx.saved_tensors
        acts, weights = saved[:6], saved[6:]
        act = ctx.act
        B, H, W, _ = acts[5].shape
        N = 2 * B
        g = gy.contiguous()
        if ctx.last:
            if act == ACT["tanh"]:
                g = g * (1.0 - acts[5] * acts[5])
            elif act == ACT["relu"]:
                g = g * (acts[5] > 0).to(g.dtype)
        grads = _tower_backward(g, _view(TOWER_PITCH, 0, 2), acts, weights, act, N, H, W)
        if BACKWARD_TRACE is not None:
            BACKWARD_TRACE.append(("tower", 4, 40, 5))
        return (None, None, None, *grads)


class RingTowerDrop(torch.autograd.Function):
    """``RingTower`` with the reference's element-wise input dropout of the pose CNN (site 1 of csrc/dropout.hip) on the 80 tower
    channels: ``forward(x, act, seed, p, *weights)``.  The fifth layer writes a compact ``[2B,H,W,40]`` map like layers 1..4 and
    ``dl_tower_wide_drop_f32`` makes the wide stem input from it (both slices times the mask, channels 80..127 zero).  The un-dropped
    map is kept: the stem must read dropped values, the tower's backward needs act' of the un-dropped ones (335 MB more than
    ``RingTower`` at 64 x 2048, B = 8).  Backward: the incoming gradient is the TRUE ``dL/dxw`` (``RingStemWide`` with
    ``dact_input = False``); ``dl_tower_wide_drop_bwd_f32`` regenerates the mask from the seed and returns layer 5's pre-activation
    gradient in the compact layout, from which layers 5..1 run as in ``RingTower``."""

    @staticmethod
    def forward(ctx, x, act, seed, p, *weights):
        B, _, H, W = x.shape
        N = 2 * B
        CH = TOWER_CHANNELS // 2
        a = x.contiguous().view(N, 4, H, W).permute(0, 2, 3, 1).contiguous()
        acts = [a]
        ws = [weight_storage(w) for w in weights]
        for i, (C, K) in enumerate(TOWER_PLAN):
            y = _empty((N, H, W, K), torch.float32, x.device)
            tower_conv(a, ws[i], y, (N, H, W, C, K), _view(C), _view(K), act=act, epilogue=EPI_ACT if act else 0)
            acts.append(y)
            a = y
        xw = _empty((B, H, W, TOWER_PITCH), torch.float32, x.device)
        _lib.check(_lib.load().dl_tower_wide_drop_f32(_ptr(a), _ptr(seed), float(p), B, H, W, CH, TOWER_PITCH, _ptr(xw), _stream()),
                   "dl_tower_wide_drop_f32")
        ctx.save_for_backward(*acts, seed, *weights)
        ctx.act, ctx.p = act, float(p)
        return xw

    @staticmethod
    def backward(ctx, gx):
        saved = ctx.saved_tensors
        acts, seed, weights = saved[:6], saved[6], saved[7:]
        act = ctx.act
        N, H, W, CH = acts[5].shape
        gx = gx.contiguous()
        g = _empty((N, H, W, CH), torch.float32, gx.device)
        _lib.check(_lib.load().dl_tower_wide_drop_bwd_f32(_ptr(gx), _ptr(acts[5]), _ptr(seed), ctx.p, int(act), N // 2, H, W, CH, TOWER_PITCH, _ptr(g),
                                                          _stream()), "dl_tower_wide_drop_bwd_f32")
        grads = _tower_backward(g, _view(CH), acts, weights, act, N, H, W)
        if BACKWARD_TRACE is not None:
            BACKWARD_TRACE.append(("tower_drop", 4, 40, 5))
        return (None, None, None, None, *grads)


class RingStemWide(torch.autograd.Function):
    """The stem behind the feature tower: conv1 (80 -> 64, 3x3, stride (1,2)) + activation + the 3x3 / stride (1,2) max-pooling on
    the tower's ``[N,H,W,128]`` buffer (channels 80..127 zero) -> ``[N,H,W/4,64]``.  conv1's weight is zero-padded to 128 input
    channels per call (295 kB), so that forward, input gradient (``dl_conv2d_dgrad_strided_nhwc_f32``) and weight gradient
    (``dl_conv2d_wgrad_nhwc_f32``) run on the direct kernels at C = 128, K = 64; the pooling kernels are those of ``RingStem``.
    Unlike the 8-channel stem this one returns an input gradient.  ``dact_input``: the returned gradient is multiplied by act' of
    the INPUT map in the input gradient's epilogue -- it is then the gradient of the tower's last pre-activation (what
    ``RingTower`` with ``last = False`` expects); False returns the true ``dL/dx``.  Channels 80..127 of it are zero either way."""

    @staticmethod
    def forward(ctx, xw, w1, act, dact_input):
        xw = xw.contiguous()
        N, H, W, P = xw.shape
        K, C = w1.shape[0], w1.shape[1]
        w = torch.zeros((K, 3, 3, P), dtype=torch.float32, device=xw.device)
        w[..., :C] = w1.detach().permute(0, 2, 3, 1)
        a = conv_nhwc(xw, w, stride=(1, 2), act=act, epilogue=EPI_ACT if act else 0)
        y, win = pool_fwd(a)
        ctx.save_for_backward(xw, a, win, w, w1)
        ctx.act, ctx.dact_input = act, bool(dact_input)
        return y

    @staticmethod
    def backward(ctx, g):
        xw, a, win, w, w1 = ctx.saved_tensors
        N, H, W, P = xw.shape
        C = w1.shape[1]
        gc = pool_bwd(g.contiguous(), a, win, ctx.act)                     # gradient of conv1's pre-activation
        # the first C input channels, dense in the parameter's own memory layout (AccumulateGrad and DDP's bucket views then take
        # the gradient as it is instead of re-laying it out every step)
        dw = wgrad_nhwc(xw, gc, 3, stride=(1, 2))[..., :C].permute(0, 3, 1, 2)
        dw = dw.contiguous(memory_format=torch.channels_last if w1.is_contiguous(memory_format=torch.channels_last) and not w1.is_contiguous()
                           else torch.contiguous_format)
        gx = None
        if ctx.needs_input_grad[0]:
            fold = ctx.dact_input and ctx.act
            gx = dgrad_strided(gc, w, (1, 2), (H, W), act=ctx.act, epilogue=EPI_DACT if fold else 0, dsrc=xw if fold else None)
        if BACKWARD_TRACE is not None:
            BACKWARD_TRACE.append(("stem_wide", C, w1.shape[0], 1))
        return gx, dw, None, None


# How the trunk is cut into autograd Functions.  Each Function hands its weight gradients to autograd when its backward has run, so
# the cuts decide what DistributedDataParallel can overlap with the rest of the backward; each Function also costs the host
# ~0.1 ms per step (apply + saved tensors + backward dispatch), and the eager step is only just GPU-bound:
#   "mono"   one Function for layer1..layer4 (single process: nothing to overlap)
#   "layer"  [layer1 + layer2] [layer3] [layer4]: layer4 (71 % of the gradient bytes) and layer3 (18 %) are in flight while the
#            rest of the backward runs -- what deploy/trainer.py selects under DDP
#   "block"  one Function per residual block
TRUNK_SEGMENTS = "mono"
# Fewest input channels of a stride-1 3x3 layer whose weight gradient takes the Winograd-domain kernel inside a merged launch.  A single
# launch keeps 128 (wgrad_nhwc): a 64-channel layer has ONE output tile, i.e. 256 slab partials of 262 KB each -- the direct kernel won.
# Merged with the other layers of the segment it needs 64 slabs, and 2.25x fewer multiplications decide (A/B in DESIGN.md 4.6).
WINO_WGRAD_MIN_C_BATCHED = int(os.environ.get("DELORA_WINO_WGRAD_MIN_C", "64"))
# The weight gradients of a segment run in merged launches at its end (wgrad_batch, wgrad_batch_h).  Deferring them keeps every
# inter-layer GRADIENT map of the segment alive until they are computed (the activations are saved tensors and alive anyway).  At B=8, 64x2048 that is ~1 GB for the 19 layers of a mono trunk; above this many
# bytes the collected layers are flushed early (one more merged launch), so that peak memory stays bounded for large batches / tall
# images (advisor, round 4).
WGRAD_PENDING_MAX_BYTES = int(os.environ.get("DELORA_WGRAD_PENDING_MAX_BYTES", str(2 << 30)))


class _PendingWgrads:
    """(gradient slot, (x, g, filter size, stride)) items of a segment's backward, flushed into ``grads`` through ``batch_fn`` (merged
    launches) at the end of the segment -- or earlier, once the gradient maps they keep alive pass ``WGRAD_PENDING_MAX_BYTES``."""

    def __init__(self, grads, meta, batch_fn):
        self.grads, self.meta, self.batch_fn = grads, meta, batch_fn
        self.items, self.bytes, self.flushes = [], 0, 0

    def append(self, item):
        self.items.append(item)
        g = item[1][1]
        self.bytes += g.numel() * g.element_size()
        if self.bytes > WGRAD_PENDING_MAX_BYTES:
            self.flush()

    def flush(self):
        if not self.items:
            return
        for (gi, _), dw in zip(self.items, self.batch_fn([it for _, it in self.items])):
            self.grads[gi] = grad_for(dw, self.meta[gi])
        self.items, self.bytes = [], 0
        self.flushes += 1


# Order in which the segment Functions finished their backward passes in this process (tests: DDP overlap) -- appended to when a list
BACKWARD_TRACE = None


def _segments(blocks, mode):
    """Index ranges [(b0, b1), ...] of the blocks each autograd Function covers."""
    nb = len(blocks)
    if mode == "block":
        return [(b, b + 1) for b in range(nb)]
    if mode == "layer":
        cuts = [b for b in range(1, nb) if blocks[b][3] and blocks[b][0] >= 128]      # first block of layer3 and of layer4
        edges = [0] + cuts + [nb]
        return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]
    return [(0, nb)]


# One convolution layer of a segment as the kernel family that runs it.  Every kind answers the same two questions through the module's
# wrappers -- ``fwd(x, act, epilogue, add)`` and the input gradient ``dgrad(g, in_hw, act, epilogue, add, dsrc, dense)`` (``add``: the
# addend of EPI_ADD, or the grid addend of EPI_ADD_GRID; ``in_hw``: the input image, asked for only by layers of a down-sampling
# block) -- and keeps in ``bwd`` the one tensor it wants back for ``dgrad`` (the direct kind: none), the fp32 kinds the raw
# parameter ``w`` too.
class _Layer:
    def __init__(self, cin, cout, ks, stride, down, w=None, bwd=None):
        self.cin, self.cout, self.ks, self.stride, self.down = cin, cout, ks, stride, down    # down: conv1 / 1x1 of a down-sampling block
        self.w, self.bwd = w, bwd

    def prepare(self, want_bwd):
        """What the layer issues itself ahead of its forward launch (the batched preparations are the segment's)."""


class _DirectLayer(_Layer):
    """fp32 direct kernels (csrc/conv.hip) on the raw weight: ``conv_nhwc``, transposed for a stride-1 input gradient; ``dgrad_strided``
    (one pass per stride phase, the shortcut's gradient added on the grid) for the layers of a down-sampling block."""

    def prepare(self, want_bwd):
        self.u = weight_storage(self.w)

    def fwd(self, x, act=0, epilogue=0, add=None):
        return conv_nhwc(x, self.u, stride=self.stride, act=act, epilogue=epilogue, add=add)

    def dgrad(self, g, in_hw, act=0, epilogue=0, add=None, dsrc=None, dense=False):
        if self.down:
            return dgrad_strided(g, weight_storage(self.w), self.stride, in_hw, act=act, epilogue=epilogue, add_grid=add, dsrc=dsrc, dense=dense)
        return conv_nhwc(g, weight_storage(self.w), act=act, epilogue=epilogue, add=add, dsrc=dsrc, transposed=True)


class _WinoLayer(_Layer):
    """fp32 stride-1 3x3 as fused Winograd F(2x2,3x3): ``wino_conv`` with ``u`` = u_fwd, ``bwd`` = u_bwd (``wino_weights_batch``, one
    launch per segment).  As conv1 of a stride-1 down-sampling block its input gradient is the direct layer's, the only one that adds
    on the grid (u_bwd is kept all the same)."""

    def fwd(self, x, act=0, epilogue=0, add=None):
        return wino_conv(x, self.u, self.cout, act=act, epilogue=epilogue, add=add)

    def dgrad(self, g, in_hw, act=0, epilogue=0, add=None, dsrc=None, dense=False):
        if self.down:
            return _DirectLayer.dgrad(self, g, in_hw, act, epilogue, add, dsrc, dense)
        return wino_conv(g, self.bwd, self.cin, act=act, epilogue=epilogue, add=add, dsrc=dsrc)


class _PairLayer(_Layer):
    """fp32 stride-(1,2) 3x3 as Winograd on the pixel-pair view: the rearranged kernel's transform is one launch of the layer's own."""

    def prepare(self, want_bwd):
        self.u, self.bwd = wino_strided_weights(self.w, self.stride, want_bwd=want_bwd)

    def fwd(self, x, act=0, epilogue=0, add=None):
        return wino_strided_conv(x, self.u, self.cout, self.stride, act=act, epilogue=epilogue)

    def dgrad(self, g, in_hw, act=0, epilogue=0, add=None, dsrc=None, dense=False):
        return wino_strided_dgrad(g, self.bwd, self.cin, self.stride, in_hw, act=act, epilogue=epilogue, add_grid=add, dsrc=dsrc)


class _NarrowLayer(_Layer):
    """fp32 layers of a narrow network, fewer than 64 channels on one side (csrc/narrow.hip), on the raw weight: 3x3 and 1x1, stride
    (1,1) and (1,2).  A stride-1 layer's input gradient is the transposed convolution (the grid of a stride-1 down-sampling block is the
    image: its addend is a plain ADD); a strided one's reads the gradient with zeros between its columns (``narrow_dgrad_strided``)."""

    def prepare(self, want_bwd):
        self.u = weight_storage(self.w)

    def fwd(self, x, act=0, epilogue=0, add=None):
        return narrow_conv(x, self.u, stride=self.stride, act=act, epilogue=epilogue, add=add)

    def dgrad(self, g, in_hw, act=0, epilogue=0, add=None, dsrc=None, dense=False):
        if tuple(self.stride) != (1, 1):
            return narrow_dgrad_strided(g, weight_storage(self.w), self.stride, in_hw, act=act, epilogue=epilogue, add_grid=add, dsrc=dsrc, dense=dense)
        if epilogue & EPI_ADD_GRID:
            epilogue = (epilogue & ~EPI_ADD_GRID) | EPI_ADD
        return narrow_conv(g, weight_storage(self.w), act=act, epilogue=epilogue, add=add, dsrc=dsrc, transposed=True)


class _HalfLayer(_Layer):
    """bf16 / fp16 kernels (csrc/convh.hip) on the prepared copies ``u`` = w_fwd, ``bwd`` = w_bwd (``weights_batch_h``, one launch per
    segment); the same split between stride-1 and down-sampling layers as ``_DirectLayer``."""

    def fwd(self, x, act=0, epilogue=0, add=None):
        return conv_nhwc_h(x, self.u, self.ks, stride=self.stride, act=act, epilogue=epilogue, add=add)

    def dgrad(self, g, in_hw, act=0, epilogue=0, add=None, dsrc=None, dense=False):
        if self.down:
            return dgrad_strided_h(g, self.bwd, self.ks, self.stride, in_hw, act=act, epilogue=epilogue, add_grid=add, dsrc=dsrc, dense=dense)
        return conv_nhwc_h(g, self.bwd, self.ks, act=act, epilogue=epilogue, add=add, dsrc=dsrc, transposed=True)


def _layer_plan(x_shape, blocks, dtype):
    """The kernel family of every layer of a segment, THE routing decision: one (kind, cin, cout, filter size, stride, down) per weight
    in weight order (conv1, conv2[, downsample]) from the input shape, the blocks, the precision and the module's switches.  fp32:
    stride-1 3x3 layers run as Winograd when ``USE_WINOGRAD`` and ``wino_ok``; conv1 of a strided down-sampling block that
    ``wino_strided_ok`` (``dl_wino_strided_takes``) accepts runs on the pixel-pair view (``USE_WINOGRAD_STRIDED``); every other layer,
    the 1x1 ones included, runs the direct kernel.  fp32 layers with fewer than 64 channels on a side (``cin % 64 or cout % 64``, a
    narrow network's first layers) run on the narrow family, whatever the switches say.  Half precision has one family."""
    plan, (N, H, W) = [], x_shape[:3]
    half = dtype != torch.float32
    for (cin, cout, stride, has_ds) in blocks:
        k1 = k2 = kd = _HalfLayer if half else _DirectLayer
        narrow1 = not half and bool(cin % 64 or cout % 64) and narrow_ok(cin, cout)
        if USE_WINOGRAD and not half and not narrow1:
            if stride == (1, 1):
                k1 = _WinoLayer if wino_ok(H, W, cin, cout) else k1
            elif USE_WINOGRAD_STRIDED and tuple(stride) != (1, 1) and has_ds and wino_strided_ok(N, H, W, cin, cout, stride):
                k1 = _PairLayer
        H, W = out_size(H, stride[0]), out_size(W, stride[1])
        if USE_WINOGRAD and not half and wino_ok(H, W, cout, cout):
            k2 = _WinoLayer
        if narrow1:
            k1 = kd = _NarrowLayer
        if not half and cout % 64 and narrow_ok(cout, cout):
            k2 = _NarrowLayer
        plan += [(k1, cin, cout, 3, stride, has_ds), (k2, cout, cout, 3, (1, 1), False)]
        if has_ds:
            plan.append((kd, cin, cout, 1, stride, True))
    return plan


def _segment_forward(ctx, plan, layers, x0, act, blocks, first, last, need_bwd, keep):
    """The forward walk of both precisions: per block conv1, shortcut, conv2 on ``layers`` (``plan`` made into objects, the batched
    weight preparations attached).  Saved for the backward pass: x0 and the two activations per block, ``keep`` (fp32: the raw
    weights), the layers' ``bwd`` tensors, the tensor ``first``; ``ctx`` itself holds no tensor."""
    saved, x, it = [x0], x0, iter(layers)
    for (_, _, _, has_ds) in blocks:
        l1, l2 = next(it), next(it)
        if has_ds:                                      # (the 1x1 weight's view is taken ahead of conv1: tests pin the call order)
            ld = next(it)
            ld.prepare(need_bwd)
        l1.prepare(need_bwd)
        y1 = l1.fwd(x, act, EPI_ACT)
        shortcut = ld.fwd(x) if has_ds else x
        l2.prepare(need_bwd)
        x = l2.fwd(y1, act, EPI_ADD | EPI_ACT, shortcut)
        saved += [y1, x]
    dsrc0 = [first] if torch.is_tensor(first) else []
    ctx.act, ctx.blocks, ctx.first, ctx.last, ctx.plan, ctx.has_dsrc0 = act, blocks, not dsrc0 and bool(first), last, plan, bool(dsrc0)
    ctx.save_for_backward(*saved, *keep, *[l.bwd for l in layers if l.bwd is not None], *dsrc0)
    return x


def _saved(ctx):
    """What ``_segment_forward`` saved: (x0 and the two activations per block, the Function's own tensors, the tensor ``first`` or None)."""
    saved, n = ctx.saved_tensors, 1 + 2 * len(ctx.blocks)
    if ctx.has_dsrc0:
        return saved[:n], saved[n:-1], saved[-1]
    return saved[:n], saved[n:], None


def _segment_backward(ctx, layers, acts, dsrc0, dy, meta, batch_fn):
    """The backward walk of both precisions on the rebuilt ``layers``: the chain of input gradients, act' and the shortcut's gradient in
    their epilogues; ``meta``: what ``grad_for`` lays the weight gradients of ``batch_fn`` out by."""
    act, blocks = ctx.act, ctx.blocks
    nb = len(blocks)
    grads = [None] * len(layers)
    g2 = dy.contiguous()
    if ctx.last:                                        # a true dL/dy: the activation derivative is applied here
        y_last = acts[-1]
        if act == ACT["tanh"] and g2.dtype == torch.float32:
            g2 = g2 * (1.0 - y_last * y_last)
        elif act == ACT["tanh"]:                        # half precision: in fp32, one rounding (never taken by ring_trunk_h, whose
            g2 = (g2.float() * (1.0 - y_last.float() ** 2)).to(g2.dtype)      # pooling hands over the pre-activation gradient)
        elif act == ACT["relu"]:
            g2 = g2 * (y_last > 0).to(g2.dtype)
    # The weight gradients do not feed the chain of input gradients: they are collected (x, g stay alive) and computed together at
    # the end of the segment -- merged launches need far fewer slab partials than one launch per layer (wgrad_batch, wgrad_batch_h)
    pending = _PendingWgrads(grads, meta, batch_fn)
    wi = len(layers)
    for b in range(nb - 1, -1, -1):
        stride, has_ds = blocks[b][2], blocks[b][3]
        wi -= 3 if has_ds else 2
        l1, l2 = layers[wi], layers[wi + 1]
        x, y1 = acts[2 * b], acts[2 * b + 1]
        # x0 of the first segment is the pooled stem output: its act' belongs to the stem.  Elsewhere the returned gradient carries
        # act' of x -- or of the map x0 was scaled from (``first`` as a tensor)
        dsrc = None if ctx.first and b == 0 else dsrc0 if b == 0 and dsrc0 is not None else x
        dact = EPI_DACT if dsrc is not None else 0
        pending.append((wi + 1, (y1, g2, 3, (1, 1))))
        g1 = l2.dgrad(g2, None, act, EPI_DACT, None, y1)
        pending.append((wi, (x, g1, 3, stride)))
        if not has_ds:
            g2 = l1.dgrad(g1, None, act, EPI_ADD | dact, g2, dsrc)
        else:
            pending.append((wi + 2, (x, g2, 1, stride)))
            # down-sampling branch on the grid, then one pass per stride phase of the 3x3 layer with it and act'(x) fused
            dxb = layers[wi + 2].dgrad(g2, x.shape[1:3], dense=True)
            g2 = l1.dgrad(g1, x.shape[1:3], act, EPI_ADD_GRID | dact, dxb, dsrc)
    pending.flush()
    if BACKWARD_TRACE is not None:
        BACKWARD_TRACE.append(("segment", blocks[0][0], blocks[-1][1], nb))
    return (g2, None, None, None, None, *grads)


class RingSegment(torch.autograd.Function):
    """A run of residual blocks of the pose CNN (reference BasicBlock.forward, src/models/resnet_modified.py:159-177) on channels-
    last fp32 activations: ``forward(x, act, blocks, first, last, *weights)`` with blocks = tuple of (cin, cout, stride,
    has_downsample) and the weights in block order (conv1, conv2[, downsample]); returns the last block's activated output.

    Private gradient convention BETWEEN two segments (the tensors never leave ``ring_trunk``): the gradient a segment receives for
    its output is already multiplied by ``act'(output)`` -- it is the gradient with respect to the PRE-activation -- because
    the consumer folds that factor into the epilogue of its input-gradient convolution (``EPI_DACT``): no elementwise kernel
    runs between two convolutions, across segment boundaries either.  Only the ``last`` segment receives a true ``dL/dy`` (from
    the pooling) and applies ``act'`` itself; only the ``first`` one returns a true ``dL/dx`` (x = the pooled stem output,
    whose activation derivative belongs to the stem).  ``first`` may also be a TENSOR: the activated map x0 was derived from by a
    per-channel scaling (``ChannelDropout``) -- the returned gradient is then multiplied by ``act'`` of THAT map in the same epilogue
    (``act'`` of a dropped map would be ``1 - (1.25 y)^2``), and the scaling's own backward is a plain multiplication."""

    @staticmethod
    def forward(ctx, x0, act, blocks, first, last, *weights):
        """Which kernel runs which layer is ``_layer_plan``'s decision.  The Winograd-domain weights of the stride-1 layers, those for
        the backward pass included, come from one launch for the segment."""
        need_bwd = any(ctx.needs_input_grad)
        plan = _layer_plan(x0.shape, blocks, torch.float32)
        layers = [kind(*shape, w) for (kind, *shape), w in zip(plan, weights)]
        wino = [l for l in layers if type(l) is _WinoLayer]            # their transformed weights in ONE launch
        for l, u in zip(wino, wino_weights_batch([l.w for l in wino], want_bwd=need_bwd)):
            l.u, l.bwd = u
        # the Winograd-domain backward weights travel with the saved tensors (released with the graph, covered by autograd's
        # in-place version check like the raw weights); layers on the direct kernel have none
        return _segment_forward(ctx, plan, layers, x0, act, blocks, first, last, need_bwd, weights)

    @staticmethod
    def backward(ctx, dy):
        acts, rest, dsrc0 = _saved(ctx)                 # rest: the raw weights, then u_bwd of the layers that have one
        u_bwd = iter(rest[len(ctx.plan):])
        layers = [kind(*shape, w, None if kind in (_DirectLayer, _NarrowLayer) else next(u_bwd)) for (kind, *shape), w in zip(ctx.plan, rest)]
        return _segment_backward(ctx, layers, acts, dsrc0, dy, rest[:len(layers)], wgrad_batch)


def _run_segments(fn, x, act, blocks, weights, mode, last_applies_act, channel_drop=None):
    """``channel_drop = (scale [N][C], b)``: ``ChannelDropout`` in front of block b -- an extra cut there in every mode.  The segment
    behind it takes the UN-dropped map as the source of the activation derivative of the gradient it returns (``first`` = that
    tensor), the dropout's backward multiplies by the scale, and the segment in front of it stays at ``last=False``: it receives a
    pre-activation gradient exactly as without the cut."""
    segs = _segments(blocks, mode or TRUNK_SEGMENTS)
    cut = None
    if channel_drop is not None:
        scale, cut = channel_drop
        if not 0 < cut < len(blocks):
            raise ValueError(f"channel dropout in front of block {cut} of {len(blocks)}")
        segs = [part for (b0, b1) in segs for part in (((b0, cut), (cut, b1)) if b0 < cut < b1 else ((b0, b1),))]
    wi = 0
    for i, (b0, b1) in enumerate(segs):
        nw = sum(3 if blocks[b][3] else 2 for b in range(b0, b1))
        first = i == 0
        if b0 == cut:
            first, x = x, ChannelDropout.apply(x, scale, 0)
        x = fn.apply(x, act, tuple(blocks[b0:b1]), first, last_applies_act and i == len(segs) - 1, *weights[wi:wi + nw])
        wi += nw
    return x


def ring_trunk(x0, act, blocks, weights, segments=None, channel_drop=None):
    """layer1..layer4 of the pose CNN: x0 ``[N,H,W,C0]`` channels-last fp32, already activated (the pooled stem output); blocks =
    tuple of (cin, cout, stride, has_downsample); weights in block order (conv1, conv2[, downsample]).  Returns the last
    feature map ``[N,H',W',C']``.  ``segments``: how the trunk is cut into autograd Functions (default ``TRUNK_SEGMENTS``).
    ``channel_drop``: (scale ``[N][C]``, block index) -- channel dropout on the input of that block (see ``_run_segments``)."""
    return _run_segments(RingSegment, x0, act, blocks, list(weights), segments, True, channel_drop)


class RingTrunk:
    """Round-2 interface kept for callers: ``RingTrunk.apply(x0, act, blocks, *weights)`` = ``ring_trunk``."""

    @staticmethod
    def apply(x0, act, blocks, *weights):
        return ring_trunk(x0, act, blocks, list(weights))


# ---------------------------------------------------------------------------------------------------------------------
# Half precision (autocast): the same trunk on v_mfma_f32_32x32x16_bf16 / _f16 (csrc/convh.hip, wgradh.hip).  Activations and
# gradients live in bf16 / fp16 channels-last, accumulation and elementwise tails are fp32, the parameters stay fp32 (their
# half-precision copies in the two layouts the kernels read are rebuilt per call), weight gradients come back in fp32.

DTYPE_CODE = {torch.float16: 1, torch.bfloat16: 2}          # DL_DTYPE_F16 / DL_DTYPE_BF16


def weights_h(w_param, dtype, want_fwd=True, want_bwd=True):
    """Half-precision copies of a convolution parameter ``[K,C,k,k]``: (w_fwd ``[k*k,K,C]``, w_bwd ``[k*k,C,K]``)."""
    lib = _lib.load()
    w = weight_storage(w_param)
    K, ks, _, C = w.shape
    wf = torch.empty((ks * ks, K, C), dtype=dtype, device=w.device) if want_fwd else None
    wb = torch.empty((ks * ks, C, K), dtype=dtype, device=w.device) if want_bwd else None
    _lib.check(lib.dl_conv_weights_h(_ptr(w), _ptr(wf), _ptr(wb), K, ks * ks, C, DTYPE_CODE[dtype], _stream()), "dl_conv_weights_h")
    return wf, wb


def weights_batch_h(w_params, dtype, want_bwd=True):
    """``weights_h`` for a list of parameters in ONE launch (``dl_conv_weights_batch_h``): list of (w_fwd, w_bwd)."""
    lib = _lib.load()
    ws = [weight_storage(w) for w in w_params]
    out = []
    for w in ws:
        K, ks, _, C = w.shape
        out.append((torch.empty((ks * ks, K, C), dtype=dtype, device=w.device),
                    torch.empty((ks * ks, C, K), dtype=dtype, device=w.device) if want_bwd else None))
    for i0 in range(0, len(ws), _lib.CONVH_BATCH):
        part = list(range(i0, min(i0 + _lib.CONVH_BATCH, len(ws))))
        arr = (_lib.ConvHLayer * len(part))()
        for j, i in enumerate(part):
            K, ks, _, C = ws[i].shape
            arr[j].w = ws[i].data_ptr()
            arr[j].w_fwd = out[i][0].data_ptr()
            arr[j].w_bwd = out[i][1].data_ptr() if want_bwd else None
            arr[j].K, arr[j].taps, arr[j].C = K, ks * ks, C
        _lib.check(lib.dl_conv_weights_batch_h(ctypes.cast(arr, ctypes.c_void_p), len(part), DTYPE_CODE[dtype], _stream()), "dl_conv_weights_batch_h")
    return out


def conv_nhwc_h(x, w_prepared, ks, stride=(1, 1), act=0, epilogue=0, add=None, dsrc=None, transposed=False):
    """``y = epilogue(conv(x, w))`` on half-precision channels-last tensors; ``w_prepared`` = ``w_fwd`` of the layer, or (``transposed``)
    ``w_bwd`` of the layer whose input gradient is wanted, x then being the output gradient."""
    lib = _lib.load()
    N, H, W, C = x.shape
    K = w_prepared.shape[1]
    y = torch.empty((N, out_size(H, stride[0]), out_size(W, stride[1]), K), dtype=x.dtype, device=x.device)
    _lib.check(lib.dl_conv2d_nhwc_h(_ptr(x), _ptr(w_prepared), _ptr(y), _ptr(add), _ptr(dsrc), N, H, W, C, K, ks, stride[0], stride[1],
                                    int(transposed), DTYPE_CODE[x.dtype], int(act), int(epilogue), _stream()), "dl_conv2d_nhwc_h")
    return y


def dgrad_strided_h(g, w_bwd, ks, stride, in_hw, act=0, epilogue=0, add_grid=None, dsrc=None, dense=False):
    """Input gradient of a strided layer whose INPUT image is ``in_hw`` = (H, W), from its half-precision output gradient
    ``[N,Ho,Wo,K]`` (Ho = ceil(H / sh), Wo = ceil(W / sw)) and ``w_bwd [k*k,C,K]`` -> ``[N,H,W,C]`` (``dense``: ``[N,Ho,Wo,C]``)."""
    lib = _lib.load()
    N, Ho, Wo, K = g.shape
    H, W = int(in_hw[0]), int(in_hw[1])
    assert Ho == out_size(H, stride[0]) and Wo == out_size(W, stride[1]), (g.shape, in_hw, stride)
    C = w_bwd.shape[1]
    shape = (N, Ho, Wo, C) if dense else (N, H, W, C)
    dx = torch.empty(shape, dtype=g.dtype, device=g.device)
    seam = _seam_workspace(N, H, W, C, ks, stride, dense, g.device)
    _lib.check(lib.dl_conv2d_dgrad_strided_nhwc_h(_ptr(g), _ptr(w_bwd), _ptr(dx), _ptr(add_grid), _ptr(dsrc), N, H, W, K, C, ks, stride[0],
                                                  stride[1], int(dense), DTYPE_CODE[g.dtype], int(act), int(epilogue), _ptr(seam), _stream()),
               "dl_conv2d_dgrad_strided_nhwc_h")
    return dx


def wgrad_nhwc_h(x, g, ks, stride=(1, 1)):
    """fp32 ``dW [K,k,k,C]`` (channels_last storage of the parameter gradient) from half-precision input x and output gradient g."""
    lib = _lib.load()
    N, H, W, C = x.shape
    K = g.shape[3]
    nbytes = lib.dl_conv2d_wgrad_h_workspace_bytes(N, H, W, C, K, ks, stride[0], stride[1])
    if not nbytes:
        raise _lib.DeloraHipError(f"dl_conv2d_wgrad_nhwc_h does not support x {tuple(x.shape)} -> K={K}, kernel {ks}, stride {stride}")
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
    dw = torch.empty((K, ks, ks, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.dl_conv2d_wgrad_nhwc_h(_ptr(x), _ptr(g), _ptr(dw), _ptr(ws), N, H, W, C, K, ks, stride[0], stride[1], DTYPE_CODE[x.dtype],
                                          _stream()), "dl_conv2d_wgrad_nhwc_h")
    return dw


def wgrad_batch_h(items):
    """The weight gradients of several layers in one call (``dl_conv2d_wgrad_batch_nhwc_h``): ``items`` = list of (x, g, ks, stride) with
    half-precision channels-last x / g; returns the fp32 ``dW [K,k,k,C]`` of every item.  Layers that share a kernel run in ONE launch
    and need far fewer pixel slabs each than a launch of their own would (include/delora_hip.h); the caller keeps x and g alive until
    the call -- ``RingSegmentH.backward`` defers the gradients of a whole segment to its end."""
    return _wgrad_batch_call(items, "dl_conv2d_wgrad_batch_h_workspace_bytes", "dl_conv2d_wgrad_batch_nhwc_h", "dl_conv2d_wgrad_batch_nhwc_h",
                             DTYPE_CODE[items[0][0].dtype])


def supported_h(x_shape, blocks):
    """Whether the half-precision HIP trunk can run these shapes: as ``supported`` (channel counts multiples of 64, any image size:
    tiles hang over the edges of feature maps that do not divide)."""
    return _supported(x_shape, blocks, 1 << 30)


class CastToHalf(torch.autograd.Function):
    """fp32 -> bf16 / fp16 copy of the pooled stem output (one launch); the backward converts the gradient back."""

    @staticmethod
    def forward(ctx, x, dtype):
        lib = _lib.load()
        x = x.contiguous()
        y = torch.empty(x.shape, dtype=dtype, device=x.device)
        _lib.check(lib.dl_cast_f32_to_h(_ptr(x), _ptr(y), x.numel(), DTYPE_CODE[dtype], _stream()), "dl_cast_f32_to_h")
        return y

    @staticmethod
    def backward(ctx, g):
        return g.float(), None


class RingSegmentH(torch.autograd.Function):
    """``RingSegment`` in half precision: x / outputs / inter-segment gradients in bf16 or fp16, fp32 parameters, fp32 weight
    gradients (same private gradient convention, same launch structure; one weight-conversion launch per segment in addition)."""

    @staticmethod
    def forward(ctx, x0, act, blocks, first, last, *weights):
        need_bwd = any(ctx.needs_input_grad)
        plan = _layer_plan(x0.shape, blocks, x0.dtype)
        layers = [kind(*shape) for kind, *shape in plan]
        for l, w in zip(layers, weights_batch_h(list(weights), x0.dtype, want_bwd=need_bwd)):      # every convolution of the segment: one launch
            l.u, l.bwd = w
        ctx.w_meta = [(tuple(w.shape), tuple(w.stride())) for w in weights]
        return _segment_forward(ctx, plan, layers, x0, act, blocks, first, last, need_bwd, ())

    @staticmethod
    def backward(ctx, dy):
        acts, w_bwd, dsrc0 = _saved(ctx)
        layers = [kind(*shape, None, w) for (kind, *shape), w in zip(ctx.plan, w_bwd)]
        return _segment_backward(ctx, layers, acts, dsrc0, dy, ctx.w_meta, wgrad_batch_h)


class MeanHWActH(torch.autograd.Function):
    """Global average pooling of the last half-precision feature map -> fp32 ``[N,C]``; its backward is fused with the activation
    derivative of the block that produced the map and returns the gradient with respect to that block's PRE-activation (the
    private convention of ``RingSegmentH``)."""

    @staticmethod
    def forward(ctx, y, act):
        lib = _lib.load()
        N, H, W, C = y.shape
        feat = torch.empty((N, C), dtype=torch.float32, device=y.device)
        _lib.check(lib.dl_mean_hw_nhwc_h(_ptr(y), N, H * W, C, DTYPE_CODE[y.dtype], _ptr(feat), _stream()), "dl_mean_hw_nhwc_h")
        ctx.save_for_backward(y)
        ctx.act = act
        return feat

    @staticmethod
    def backward(ctx, gfeat):
        lib = _lib.load()
        (y,) = ctx.saved_tensors
        N, H, W, C = y.shape
        g = torch.empty_like(y)
        _lib.check(lib.dl_mean_hw_bwd_act_h(_ptr(gfeat.contiguous().float()), _ptr(y), N, H * W, C, ctx.act, DTYPE_CODE[y.dtype], _ptr(g),
                                            _stream()), "dl_mean_hw_bwd_act_h")
        return g, None


def ring_trunk_h(x0, act, blocks, dtype, weights, segments=None, channel_drop=None, x0_is_half=False):
    """layer1..layer4 + global average pooling in half precision: x0 ``[N,H,W,C0]`` fp32 channels-last (the pooled stem output),
    fp32 parameters in block order; returns the pooled features ``[N,C']`` in fp32.  ``x0_is_half``: x0 is already in ``dtype`` (the
    output of ``RingStemH``) -- no ``CastToHalf`` launch, and the first segment's input gradient goes back in half as it is."""
    if x0_is_half:
        if x0.dtype != dtype:
            raise TypeError(f"ring_trunk_h(x0_is_half=True): x0 is {x0.dtype}, the trunk runs in {dtype}")
    else:
        x0 = CastToHalf.apply(x0, dtype)
    x = _run_segments(RingSegmentH, x0, act, blocks, list(weights), segments, False, channel_drop)
    return MeanHWActH.apply(x, act)


def stem_input_h(x, dtype):
    """The planar fp32 image ``[N,8,H,W]`` as channels-last half ``[N,H,W,8]`` (``dl_stem_input_nhwc_h``: one transposing, rounding copy)."""
    lib = _lib.load()
    x = x.contiguous()
    N, C, H, W = x.shape
    x8h = torch.empty((N, H, W, 8), dtype=dtype, device=x.device)
    _lib.check(lib.dl_stem_input_nhwc_h(_ptr(x), N, H, W, DTYPE_CODE[dtype], _ptr(x8h), _stream()), "dl_stem_input_nhwc_h")
    return x8h


def stem_conv1_h(x8h, w1, act):
    """conv1 + activation on the half image: ``a [N,H,W/2,64]`` in the dtype of ``x8h``; ``w1`` the raw fp32 parameter ``[64,8,3,3]``."""
    lib = _lib.load()
    N, H, W, _ = x8h.shape
    a = torch.empty((N, H, W // 2, 64), dtype=x8h.dtype, device=x8h.device)
    _lib.check(lib.dl_stem_conv1_h(_ptr(x8h), _ptr(weight_storage(w1)), N, H, W, int(act), DTYPE_CODE[x8h.dtype], _ptr(a), _stream()),
               "dl_stem_conv1_h")
    return a


def pool_fwd_h(a):
    """Stem max-pooling of a half map ``[N,H,Wc,C]`` -> (y ``[N,H,Wc/2,C]`` in the same dtype, win int8)."""
    lib = _lib.load()
    N, H, Wc, C = a.shape
    y = torch.empty((N, H, Wc // 2, C), dtype=a.dtype, device=a.device)
    win = torch.empty((N, H, Wc // 2, C), dtype=torch.int8, device=a.device)
    _lib.check(lib.dl_stem_pool_fwd_h(_ptr(a), N, H, Wc, C, DTYPE_CODE[a.dtype], _ptr(y), _ptr(win), _stream()), "dl_stem_pool_fwd_h")
    return y, win


def stem_h_supported(x_shape, out_channels):
    """Whether ``RingStemH`` takes a planar input ``[N,8,H,W]``: the 8 -> 64 conv1, a width that halves twice, fewer than 2^31 elements
    in conv1's output."""
    N, C, H, W = x_shape
    return C == 8 and out_channels == 64 and W % 4 == 0 and W >= 4 and H >= 1 and N >= 1 and N * H * W * 32 < (1 << 31)


class RingStemH(torch.autograd.Function):
    """``RingStem`` in half precision (csrc/stemh.hip): ``RingStemH.apply(x, w1, act, dtype)`` with the planar fp32 image ``[N,8,H,W]``
    and the fp32 parameter ``w1 [64,8,3,3]`` -> the pooled map ``[N,H,W/4,64]`` in ``dtype``.  Forward: the rounding, transposing copy
    (``x8h``), conv1 + activation on the half-precision MFMA with fp32 accumulation (``a``), the pooling on the half map (``y``, ``win``).
    Saved: ``x8h``, ``a``, ``win``, ``w1`` -- half of what ``RingStem`` keeps.  Backward: the half gradient of ``y`` -> ``dw`` (fp32, laid
    out as the parameter) in one fused launch pair, ``dl_stem_wgrad_h``.  The image gets NO gradient: callers keep inputs that require
    one on the fp32 stem (``ResNetModified.hip_half_stem_applicable``), and asking for it here is an error, not a silent zero."""

    @staticmethod
    def forward(ctx, x, w1, act, dtype):
        if not stem_h_supported(tuple(x.shape), w1.shape[0]) or x.dtype != torch.float32 or w1.dtype != torch.float32:
            raise _lib.DeloraHipError(f"RingStemH does not take x {tuple(x.shape)} {x.dtype}, w1 {tuple(w1.shape)} {w1.dtype}")
        if ctx.needs_input_grad[0]:
            raise _lib.DeloraHipError("RingStemH computes no gradient with respect to the image; use RingStem")
        x8h = stem_input_h(x, dtype)
        a = stem_conv1_h(x8h, w1, act)
        y, win = pool_fwd_h(a)
        ctx.save_for_backward(x8h, a, win, w1)
        ctx.act = int(act)
        return y

    @staticmethod
    def backward(ctx, g):
        x8h, a, win, w1 = ctx.saved_tensors
        lib = _lib.load()
        N, H, W, _ = x8h.shape
        nbytes = lib.dl_stem_wgrad_h_workspace_bytes(N, H, W)
        if not nbytes:
            raise _lib.DeloraHipError(f"dl_stem_wgrad_h does not support x8h {tuple(x8h.shape)}")
        if g.dtype != a.dtype:
            g = g.to(a.dtype)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x8h.device)
        dw = torch.empty((64, 8, 3, 3), dtype=torch.float32, device=x8h.device)
        _lib.check(lib.dl_stem_wgrad_h(_ptr(g.contiguous()), _ptr(a), _ptr(win), _ptr(x8h), N, H, W, ctx.act, DTYPE_CODE[a.dtype], _ptr(ws),
                                       _ptr(dw), _stream()), "dl_stem_wgrad_h")
        return None, (dw if tuple(dw.stride()) == tuple(w1.stride()) else grad_for(dw.permute(0, 2, 3, 1).contiguous(), w1)), None, None


class RingTrunkH:
    """``RingTrunkH.apply(x0, act, blocks, dtype, *weights)`` = ``ring_trunk_h`` (interface of the first version, one Function)."""

    @staticmethod
    def apply(x0, act, blocks, dtype, *weights):
        return ring_trunk_h(x0, act, blocks, dtype, list(weights))
