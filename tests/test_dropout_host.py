"""Host side of the dropout on the HIP path: the numpy replica of the library's random stream (the contract of include/delora_hip.h:
Philox4x32-10, counter = (i >> 2, i >> 34, site, 0), key = the 64-bit seed, decision i reads word i & 3, dropped iff word <
round(p 2^32)) against published known answers; the segment cut the channel dropout adds; and the module path (``cnn_impl: modules``),
which keeps torch's dropout modules and must be untouched.  The replica is what tests/test_gpu_dropout.py compares the kernels with."""
import numpy as np
import torch

from tests import util

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
SITE_INPUT, SITE_CHANNELS, SITE_FC = 1, 2, 3


def philox4x32(ctr, key, rounds=10):
    """Philox4x32 of Salmon et al. (Random123): ctr = four uint32 words (arrays broadcast), key = two; returns four uint64 arrays < 2^32."""
    mask = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & mask for x in ctr]
    k = [np.uint64(key[0]), np.uint64(key[1])]
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return c


def site_words(seed, site, n):
    """The n 32-bit words decision 0 .. n-1 of a site read (uint64 array)."""
    seed = int(seed) & (2 ** 64 - 1)
    quads = np.arange((n + 3) // 4, dtype=np.uint64)
    out = philox4x32((quads & np.uint64(0xFFFFFFFF), quads >> np.uint64(32), np.full_like(quads, site), np.zeros_like(quads)),
                     (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1).reshape(-1)[:n]


def site_scales(seed, site, n, p=0.2):
    """fp32 scale of every decision: 0 where dropped, 1.0f / (1.0f - p) where kept."""
    thresh = int(round(float(p) * 2.0 ** 32))
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(site_words(seed, site, n) < np.uint64(thresh), np.float32(0.0), keep).astype(np.float32)


def test_philox_replica_reproduces_the_known_answers():
    """Counter 0 / key 0 and the pi-digits vector are the published Random123 known answers of philox4x32-10; all ones is the third."""
    kat = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        assert " ".join("%08x" % int(v) for v in philox4x32(ctr, key)) == want


def test_replica_decisions_thresholds_and_rates():
    assert int(round(0.2 * 2.0 ** 32)) == 0x33333333
    s = site_scales((7 << 32) | 1234, SITE_CHANNELS, 2048)
    assert set(np.unique(s).tolist()) == {0.0, 1.25}
    assert np.all(site_scales(99, SITE_FC, 1000, p=0.0) == np.float32(1.0))
    # decision i reads word i & 3 of the call for quad i >> 2: a prefix of a longer stream is the shorter stream
    assert np.array_equal(site_scales(5, SITE_INPUT, 5), site_scales(5, SITE_INPUT, 4096)[:5])
    # sites and seeds (either half of the key) give different streams
    a = site_words(1234, SITE_CHANNELS, 256)
    assert not np.array_equal(a, site_words(1234, SITE_FC, 256)) and not np.array_equal(a, site_words(1234 + (1 << 32), SITE_CHANNELS, 256))
    for n in (2048, 8000, 1 << 20):                # keep rate within 6 sigma of 0.8
        keep = float((site_scales((7 << 32) | 1234, SITE_INPUT, n) > 0).mean())
        assert abs(keep - 0.8) <= 6.0 * np.sqrt(0.16 / n), (n, keep)


def test_channel_dropout_adds_one_cut_in_every_segment_mode(monkeypatch):
    """``_run_segments`` with a channel dropout in front of block 6 (layer4.0 of the 2-2-2-2 network): every mode gets a cut there, the
    segment behind it is handed the un-dropped map as ``first`` (the source of its gradient's activation derivative), the one in front
    of it keeps last=False, and the weights are dealt out in block order."""
    from delora_amd.models import ring_conv as rc
    blocks = ((64, 64, (1, 1), False), (64, 64, (1, 1), False), (64, 128, (1, 2), True), (128, 128, (1, 1), False),
              (128, 256, (1, 2), True), (256, 256, (1, 1), False), (256, 512, (2, 2), True), (512, 512, (1, 1), False))
    weights = list(range(sum(3 if b[3] else 2 for b in blocks)))
    calls = []

    class Seg:
        @staticmethod
        def apply(x, act, blks, first, last, *w):
            calls.append(("seg", len(blks), blks[0][0], first, last, w))
            return x

    class Drop:
        @staticmethod
        def apply(x, scale, act):
            calls.append(("drop", scale))
            assert act == 0
            return "dropped"

    monkeypatch.setattr(rc, "ChannelDropout", Drop)
    for mode, n_plain, n_cut in (("mono", 1, 2), ("layer", 3, 3), ("block", 8, 8)):
        calls.clear()
        rc._run_segments(Seg, "x0", 1, blocks, weights, mode, True)
        assert [c[0] for c in calls] == ["seg"] * n_plain and [c[3] for c in calls] == [True] + [False] * (n_plain - 1)
        calls.clear()
        rc._run_segments(Seg, "x0", 1, blocks, weights, mode, True, channel_drop=("S", 6))
        segs = [c for c in calls if c[0] == "seg"]
        assert len(segs) == n_cut and sum(c[1] for c in segs) == 8
        i = calls.index(("drop", "S"))
        assert calls[i + 1][2] == 256 and calls[i + 1][3] == "x0"            # layer4.0 follows the dropout; act' from the un-dropped map
        assert calls[i - 1][4] is False                                       # layer3's segment still expects a pre-activation gradient
        assert [c[3] for c in segs].count(True) == 1 and segs[-1][4] is True and [c[4] for c in segs[:-1]] == [False] * (n_cut - 1)
        assert [v for c in segs for v in c[5]] == weights


def test_rank_mixing_changes_the_seed_per_rank_only_under_several_ranks():
    from delora_amd.models import ring_conv as rc
    seed = torch.tensor([0x1234_5678_9ABC], dtype=torch.int64)
    assert rc.mix_rank(seed, 0, 1) is seed
    mixed = [int(rc.mix_rank(seed, r, 2)) for r in (0, 1)]
    assert len({int(seed), *mixed}) == 3


def _narrow(use_dropout):
    from delora_amd.models.model import OdometryModel
    cfg = util.repo_config(16, 128, device="cpu", factor_fewer_resnet_channels=8, resnet_outputs=64, use_dropout=use_dropout, cnn_impl="modules")
    torch.manual_seed(4)
    return OdometryModel(cfg)


def test_module_path_keeps_torch_dropout_on_the_cpu():
    """``cnn_impl: modules`` with ``use_dropout: True``: training mode draws new masks on every call; eval mode equals the model
    built without dropout bit for bit."""
    m_drop, m_plain = _narrow(True), _narrow(False)
    m_plain.load_state_dict(m_drop.state_dict())
    x = torch.randn((2, 8, 16, 128), generator=torch.Generator().manual_seed(1))
    m_drop.train()
    with torch.no_grad():
        t1, q1 = m_drop(x)
        t2, q2 = m_drop(x)
    assert not torch.equal(t1, t2) and not torch.equal(q1, q2)
    assert not hasattr(m_drop.resnet, "last_dropout")
    m_drop.eval(), m_plain.eval()
    with torch.no_grad():
        (te, qe), (tp, qp) = m_drop(x), m_plain(x)
    assert torch.equal(te, tp) and torch.equal(qe, qp)
    m_plain.train()
    with torch.no_grad():
        tt, qt = m_plain(x)
    assert torch.equal(tt, tp) and torch.equal(qt, qp)
