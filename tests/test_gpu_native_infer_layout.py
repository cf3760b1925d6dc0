"""The documented layout of the ``prepared`` buffer (include/delora_hip.h: dl_pose_net_prepare, dl_pose_net_prepare_h), array by array:
a caller who fills or reads the buffer himself goes by the header, and the forward walk reads it at the same offsets.  fp32: the
Winograd-domain weights of the Winograd layers in block order (w1 of the stride-1 blocks, then w2), ``dl_wino_weights_floats`` floats each,
no padding.  Half precision: w_fwd [taps][K][C] of every trunk convolution in the order w1, w2, wd per block, each rounded up to 256 bytes.
Every range is compared bit for bit with what the Python path's own weight transform makes from the same parameter.  Reference network,
B = 1, 16 x 128 (the layout does not depend on the image)."""
import pytest
import torch

from delora_amd import _lib
from delora_amd.deploy import native_infer
from delora_amd.models import ring_conv
from tests.test_gpu_native_infer import _model

pytestmark = pytest.mark.gpu

B, H, W = 1, 16, 128


def _trunk():
    """(model, [(name, parameter, is 3x3 at stride 1)] in the order w1, w2, wd per block)."""
    model = _model(H, W, "tanh")[0]
    blocks, weights = model.resnet._trunk_blocks()
    layers, wi = [], 0
    for i, (_, _, stride, has_ds) in enumerate(blocks):
        layers.append((f"blocks[{i}].w1", weights[wi], tuple(stride) == (1, 1)))
        layers.append((f"blocks[{i}].w2", weights[wi + 1], True))
        if has_ds:
            layers.append((f"blocks[{i}].wd", weights[wi + 2], False))
        wi += 3 if has_ds else 2
    assert wi == len(weights) == 19
    return model, layers


def test_fp32_prepared_is_the_winograd_weights_in_block_order_without_padding():
    lib = _lib.load()
    model, layers = _trunk()
    net = native_infer.NativePoseNet(model, B, H, W)
    assert net.prepared.dtype == torch.float32
    off, seen = 0, 0
    for name, w, wino in layers:
        if not wino:
            continue
        K, C = w.shape[0], w.shape[1]
        n = int(lib.dl_wino_weights_floats(K, C))
        want = ring_conv.wino_weights_batch([w.detach()], want_bwd=False)[0][0]
        assert want.numel() == n, name
        assert torch.equal(net.prepared[off:off + n], want), (name, off)
        off += n
        seen += 1
    assert seen == 13 and 4 * off == net.prepared_bytes          # the ranges tile the buffer exactly


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16), ids=("bf16", "fp16"))
def test_half_prepared_is_every_trunk_weight_in_weight_order_at_256_byte_offsets(dtype):
    model, layers = _trunk()
    net = native_infer.NativePoseNet(model, B, H, W, dtype=dtype)
    assert net.prepared.dtype == torch.uint8
    off = 0
    for name, w, _ in layers:
        want = ring_conv.weights_batch_h([w.detach()], dtype, want_bwd=False)[0][0]
        K, C, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
        assert tuple(want.shape) == (taps, K, C), name
        n = 2 * taps * K * C
        assert off % 256 == 0
        assert torch.equal(net.prepared[off:off + n], want.reshape(-1).view(torch.uint8)), (name, off)
        off += (n + 255) // 256 * 256                                # (padding bytes between arrays are not part of the contract)
    assert off == net.prepared_bytes
