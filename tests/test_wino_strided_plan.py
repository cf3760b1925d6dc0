"""``dl_wino_strided_takes``: which strided 3x3 layers the dispatch hands to the pixel-pair Winograd kernel.  Pure host arithmetic when a
CU count is given, so it runs without a GPU."""
import pytest

CUS = 256
# (N, H, W, C, K, stride) of the strided blocks' conv1 at BASELINE's 64x2048 image (the trunk sees the pooled 64x512 map)
LAYER2_0 = (64, 512, 64, 128, (1, 2))
LAYER3_0 = (64, 256, 128, 256, (1, 2))
LAYER4_0 = (64, 128, 256, 512, (2, 2))


def _takes(N, H, W, C, K, stride, cus=CUS):
    from delora_amd import _lib
    return _lib.load().dl_wino_strided_takes(N, H, W, C, K, stride[0], stride[1], cus)


@pytest.mark.parametrize("layer", [LAYER2_0, LAYER3_0], ids=["layer2.0", "layer3.0"])
def test_baseline_stride_12_layers_are_taken_at_batch_8(layer):
    assert _takes(8, *layer) == 1


def test_layer4_0_stays_on_the_direct_kernel():
    """Stride (2,2) is not built: the query must not claim a launch no kernel runs."""
    assert _takes(8, *LAYER4_0) == 0


@pytest.mark.parametrize("layer", [LAYER2_0, LAYER3_0], ids=["layer2.0", "layer3.0"])
def test_batch_1_is_left_alone(layer):
    """At batch 1 the stride-1 dispatch would split the channels over idle CUs; one range per launch would leave most of the chip idle."""
    assert _takes(1, *layer) == 0
    assert _takes(1, *layer, cus=1) == 1            # (the shape itself tiles: a one-CU device has nothing to split over)


def test_shapes_that_do_not_tile_are_refused():
    assert _takes(8, 64, 180, 64, 128, (1, 2)) == 0          # 64x720: the 180-wide map's pair view has 45 tile columns
    assert _takes(8, 64, 90, 128, 256, (1, 2)) == 0          # 90 wide: no whole 2x2 tiles of pixel pairs
    assert _takes(8, 32, 45, 256, 512, (2, 2)) == 0          # the 45-pixel map
    assert _takes(8, 64, 2048, 8, 64, (1, 2)) == 0           # the stem: 8 input channels
    assert _takes(8, 64, 512, 64, 128, (1, 1)) == 0 and _takes(8, 64, 512, 64, 128, (2, 1)) == 0
    assert _takes(8, 63, 512, 64, 128, (1, 2)) == 0          # odd height
    assert _takes(0, 64, 512, 64, 128, (1, 2)) == 0


def test_the_answer_follows_the_cu_count():
    # 2 x 8 x 128: 4 tile groups x 2 channel blocks; split on 256 CUs, whole on one
    assert _takes(2, 8, 128, 64, 128, (1, 2), 256) == 0 and _takes(2, 8, 128, 64, 128, (1, 2), 1) == 1
