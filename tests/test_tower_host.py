"""Shape gates of the HIP feature tower and the workspace query of the narrow family: host logic, no GPU."""
import torch

from tests import util


def _model(**over):
    from delora_amd.models.model import OdometryModel
    return OdometryModel(util.repo_config(64, 720, **over))


def test_tower_and_stem_gates():
    from delora_amd.models import ring_conv as rc
    assert rc.tower_supported((2, 8, 64, 720)) and rc.tower_supported((8, 8, 64, 2048)) and rc.tower_supported((1, 8, 1, 4))
    assert not rc.tower_supported((2, 4, 64, 720)) and not rc.tower_supported((2, 80, 64, 720))
    assert not rc.tower_supported((64, 8, 128, 2048))                      # the wide buffer would pass 2^31 elements
    assert rc.stem_supported((2, 8, 64, 720), 64) and rc.stem_supported((2, 80, 64, 720), 64)
    assert not rc.stem_supported((2, 80, 64, 722), 64) and not rc.stem_supported((2, 8, 64, 722), 64)
    assert not rc.stem_supported((2, 16, 64, 720), 64) and not rc.stem_supported((2, 80, 64, 720), 8)
    # the planar 8-channel stem keeps its domain
    assert rc.planar_stem_supported((2, 8, 64, 720), 64) and not rc.planar_stem_supported((2, 80, 64, 720), 64)


def test_hip_path_takes_knows_the_networks_own_input_channels():
    plain, tower = _model(), _model(pre_feature_extraction=True)
    assert plain.resnet.conv1.in_channels == 8 and tower.resnet.conv1.in_channels == 80
    for m, c in ((plain, 8), (tower, 80)):
        takes = m.resnet.hip_path_takes
        assert takes(64, 720) and takes(64, 2048) and takes(16, 100) and not takes(64, 722) and not takes(64, 721)
        assert takes(64, 720, in_channels=c) and not takes(64, 722, in_channels=c)
    assert plain.resnet.hip_path_takes(64, 720, in_channels=80) and tower.resnet.hip_path_takes(64, 720, in_channels=8)
    narrow = _model(pre_feature_extraction=True, factor_fewer_resnet_channels=8, resnet_outputs=64)
    assert not narrow.resnet.hip_path_takes(64, 720)
    modules = _model(pre_feature_extraction=True, cnn_impl="modules")
    assert not modules.resnet.hip_path_takes(64, 720)


def test_cpu_tensors_and_other_configurations_keep_the_module_path():
    """``wide_path_dtype`` is the run-time gate: a CPU tensor, a narrow network, ``cnn_impl: modules`` and active dropout say None."""
    x = torch.zeros((1, 8, 16, 128))
    for over in (dict(), dict(factor_fewer_resnet_channels=8, resnet_outputs=64), dict(cnn_impl="modules"), dict(use_dropout=True)):
        m = _model(pre_feature_extraction=True, **over)
        assert m.resnet.wide_path_dtype(x) is None
    assert _model().resnet.wide_path_dtype(x) is None
    # parameter names of the reference's tower (src/models/model.py:31-48) are those of the state_dict
    names = set(_model(pre_feature_extraction=True).state_dict())
    assert {f"feature_extractor.{i}.weight" for i in (1, 4, 7, 10, 13)} <= names


def test_workspace_query_is_zero_for_refused_shapes():
    from delora_amd import _lib
    lib = _lib.load()
    ws = lib.dl_tower_wgrad_workspace_bytes
    for C, K in ((4, 8), (8, 16), (16, 24), (24, 32), (32, 40), (64, 64)):
        b = ws(16, 64, 2048, C, K)
        assert b > 0 and b % (K * 9 * C * 4) == 0 and b // (K * 9 * C * 4) <= 512, (C, K, b)
    assert ws(2, 64, 720, 32, 40) > 0 and ws(3, 1, 4, 4, 8) == 8 * 9 * 4 * 4          # three rows: one slab, one partial dW
    for C, K in ((6, 8), (4, 12), (4, 72), (68, 8), (0, 8), (4, 0)):
        assert ws(2, 16, 128, C, K) == 0, (C, K)
    assert ws(0, 16, 128, 4, 8) == 0 and ws(2, 0, 128, 4, 8) == 0 and ws(2, 16, 0, 4, 8) == 0
    assert ws(1 << 14, 64, 2048, 4, 8) == 0                                   # beyond the 32-bit offsets
