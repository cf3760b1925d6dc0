"""Exact distance ties in the exact search (dl_nn_correspond): "ties resolve to the lower pixel index" in every regime.

The scenes of tests/util.py (mirror_scene, ground_sources) put every coordinate on a 2^-10 m grid, so the kernel's fp64
distances and the float64 referee (util.nn_referee) are the same numbers, and a target and its mirror image about a plane through
the query are an exact tie.  Every comparison here is exact: zero mismatches, no slack.  The search's work lists are read back from
a caller-owned workspace, so each case knows which regime of the search served which query and asserts that the regime it is
about was reached and held ties -- including queries whose pass-A candidate was the HIGHER-index member of a tie (the case a walk
seeded without pass A's index gets wrong).
"""
import math

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

# regimes of one query (nn.hip: pass A, the three lists of pass B, the per-query pyramid walk, the two kinds of packets)
PASS_A, SCAN16, WALK16, WALK_WAVE, PYRAMID, PACKET, WPACKET = range(7)
REGIME_NAMES = ("pass A", "scan16", "tile walk 16 lanes", "tile walk one wave", "pyramid walk", "packet walk", "windowed packet")
NN_VIS0, NN_SEED_MIN, NN_PACKET_FEW, NN_PACKET_WINDOWED, NN_REC_WPACKET = 64, 8192, 1024, 4096, 0x40000000
_REC = np.dtype([("d2", "<f8"), ("slot", "<i4"), ("idx", "<i4"), ("q", "<f4", (3,)), ("rows", "<u4"), ("cols", "<u4"), ("b", "<i4")])
_PKT = np.dtype([("b", "<i4"), ("tile", "<i4"), ("mask", "<u8")])


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _geo():
    from delora_amd import geometry
    return geometry


def decode_regimes(ws, B, H, W):
    """Which part of the search served every source pixel, read from the workspace of one dl_nn_correspond call (layout of
    carve_nn in nn.hip).  Returns (counters [6], regime [B*HW] int8, pass-A candidate [B*HW] int64 (-2: not recorded), its d2,
    bound window size in pixels (0: not recorded))."""
    raw = ws.cpu().numpy().view(np.uint8)
    cnt = raw[:24].view(np.int32).copy()
    HW = H * W
    ntr, ntc = -(-H // 4), -(-W // 16)
    ntiles, nsup = ntr * ntc, -(-ntr // 4) * -(-ntc // 8)
    hdr = ((NN_VIS0 + 32 * B) * 4 + 255) // 256 * 256
    rec_bytes = B * HW * _REC.itemsize
    hard = raw[hdr:hdr + rec_bytes].view(_REC)
    mid = raw[hdr + rec_bytes:hdr + 2 * rec_bytes].view(_REC)
    off = hdr + 2 * rec_bytes + 16 * B * (3 * ntiles + 3 * nsup)
    packets = raw[off:off + 16 * B * ntiles].view(_PKT)
    windowed = cnt[5] >= NN_PACKET_WINDOWED
    regime = np.full(B * HW, PASS_A, dtype=np.int8)
    a_idx = np.full(B * HW, -2, dtype=np.int64)
    a_d2 = np.full(B * HW, np.nan)
    window = np.zeros(B * HW, dtype=np.int64)

    def place(recs, codes):
        s = recs["slot"].astype(np.int64)
        assert np.all((s >= 0) & (s < B * HW)) and np.all(regime[s] == PASS_A), "a query in two work lists"
        regime[s] = codes
        a_idx[s] = recs["idx"]
        a_d2[s] = recs["d2"]
        window[s] = ((recs["rows"] >> 16) - (recs["rows"] & 0xFFFF) + 1).astype(np.int64) * ((recs["cols"] >> 16) + 1)

    def wflag(recs):
        return windowed & ((recs["b"] & NN_REC_WPACKET) != 0)

    h0, h1, h2 = hard[:cnt[0]], hard[B * HW - cnt[1]:] if cnt[1] else hard[:0], mid[:cnt[2]]
    wpx0 = ((h0["rows"] >> 16) - (h0["rows"] & 0xFFFF) + 1).astype(np.int64) * ((h0["cols"] >> 16) + 1)
    place(h0, np.where(wflag(h0), WPACKET, np.where((wpx0 > NN_SEED_MIN) & (nsup <= 256), PYRAMID, WALK_WAVE)))
    place(h1, SCAN16)
    place(h2, np.where(wflag(h2), WPACKET, WALK16))
    pk = packets[:cnt[3]]
    k, lanes = np.nonzero((pk["mask"][:, None] >> np.arange(64, dtype=np.uint64)[None]) & np.uint64(1))
    tr, tc = pk["tile"][k].astype(np.int64) // ntc, pk["tile"][k].astype(np.int64) % ntc
    s = pk["b"][k].astype(np.int64) * HW + (tr * 4 + lanes // 16) * W + tc * 16 + lanes % 16
    assert np.all(regime[s] == PASS_A), "a query in a packet and a work list"
    regime[s] = PACKET if cnt[3] >= NN_PACKET_FEW else PYRAMID
    return cnt[:6], regime, a_idx, a_d2, window


def tie_images(H, W, family, seed=0):
    """(sensor, target image4 [1,4,H,W], source image4 [1,4,H,W]) of a mirror scene, both projected on the GPU."""
    dev = _dev()
    vfov, hfov = util.tie_sensor_fov()
    sensor = _geo().Sensor(H, W, vfov, hfov)
    tgt, src = util.mirror_scene(H, W, family, seed=seed), util.ground_sources(H, W, seed=seed)
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([tgt, src], axis=1))).to(dev)
    offs = torch.tensor([0, tgt.shape[1], tgt.shape[1] + src.shape[1]], dtype=torch.int32, device=dev)
    out = _geo().project(pts, offs, max(tgt.shape[1], src.shape[1]), sensor)
    return sensor, out["image4"][0:1].contiguous(), out["image4"][1:2].contiguous()


def run_search(sensor, tgt_imgs, src_imgs, T):
    """One batched search with a caller-owned workspace; target 'normals' are a distinct pattern so that the gathered match planes
    3..5 are checked too.  Returns (nn [B,HW] int64 cpu, match [B,6,HW] cpu, target normals [B,3,HW] cpu, decoded regimes)."""
    B, H, W = T.shape[0], sensor.H, sensor.W
    dev = tgt_imgs.device
    g = torch.Generator(device="cpu").manual_seed(7)
    tn = torch.rand((B, 3, H, W), generator=g).to(dev) + 0.5
    ws = torch.zeros((_geo().nn_workspace_bytes(B, H, W) // 8 + 1,), dtype=torch.int64, device=dev)
    nn, _, match = _geo().nn_correspond(src_imgs, None, _geo().pack_image(tgt_imgs), _geo().pack_image(tn), T.to(dev), sensor,
                                        need_without_normals=True, workspace=ws)
    torch.cuda.synchronize()
    return (nn.reshape(B, -1).long().cpu(), match.reshape(B, 6, -1).cpu(), tn.reshape(B, 3, -1).cpu(),
            decode_regimes(ws, B, H, W))


def check_match(nn_b, match_b, tgt_img, tn_b):
    """``match`` is a gather of the target image (and normals) at the returned pixel, zero where there is none."""
    tflat = tgt_img[:3].reshape(3, -1).cpu()
    ok = nn_b >= 0
    assert torch.equal(match_b[:3, ok], tflat[:, nn_b[ok]]) and torch.equal(match_b[3:, ok], tn_b[:, nn_b[ok]])
    assert (match_b[:, ~ok] == 0).all()


def regime_stats(sensor, tgt_imgs, src_imgs, T, nn, regime, a_idx, a_d2):
    """Per-sample exact comparison with the float64 referee.  Returns {regime: [queries, exact ties, exposed ties, mismatches]}
    summed over the batch; 'exposed' = pass A handed pass B the higher-index member of an exact tie."""
    B, HW = T.shape[0], sensor.H * sensor.W
    dev = tgt_imgs.device
    stats = {r: [0, 0, 0, 0] for r in range(len(REGIME_NAMES))}
    for b in range(B):
        tb, sb = tgt_imgs[b if tgt_imgs.shape[0] > 1 else 0], src_imgs[b if src_imgs.shape[0] > 1 else 0]
        tp, _, tpix = util.lists_from_images(tb, torch.zeros(3, sensor.H, sensor.W))
        sp, _, spix = util.lists_from_images(sb, torch.zeros(3, sensor.H, sensor.W))
        Td = T[b].double()
        q = Td[:3, :3] @ sp[0].double() + Td[:3, 3:]
        ref, d2, ties = (x.cpu() for x in util.nn_referee(q.to(dev), tp[0].to(dev), tpix))
        got = nn[b][spix]
        slots = b * HW + spix.numpy()
        reg = regime[slots]
        exposed = (a_idx[slots] >= 0) & (a_d2[slots] == d2.numpy()) & (a_idx[slots] > ref.numpy())
        bad = (got != ref).numpy()
        for r in range(len(REGIME_NAMES)):
            m = reg == r
            st = stats[r]
            st[0] += int(m.sum()); st[1] += int((ties.numpy()[m] >= 2).sum()); st[2] += int(exposed[m].sum()); st[3] += int(bad[m].sum())
    return stats


def describe(stats, counters):
    rows = [f"counters {list(int(c) for c in counters)}"]
    for r, (n, t, e, bad) in stats.items():
        if n:
            rows.append(f"  {REGIME_NAMES[r]:20s} queries {n:7d}  ties {t:7d}  exposed {e:6d}  mismatches {bad:6d}")
    return "\n".join(rows)


Z = util.MIRROR_Z
# name -> (H, W, family, poses, {regime: minimum number of exact ties in it}).  Which pose reaches which regime was measured on an
# MI355X with these scenes (the counts in the comments: queries of the regime, all of them exact ties; "exposed": pass A handed
# the walk the higher-index member of the tie -- the kernel before the fix got every one of those wrong).
CASES = {
    # 64 x 512, the room shifted by (0.25, -0.125): 115 queries certified by pass A, 590 scanned (68 exposed), 2613 on the 16-lane
    # tile walk (97 exposed); the rest are packets, too few for the packet walk: per-query pyramid walks
    "pass_a_and_lists": (64, 512, "ground", [(0, (0.25, -0.125, 0.0))], {PASS_A: 50, SCAN16: 300, WALK16: 1300}),
    # 32 x 512, batch 3, yaws of 90 / 180 / 270 degrees, one 25 m away: 250 source tiles, no packet walk possible; 15k queries walk
    # the pyramid one by one (the unfixed kernel: 38 of them wrong), 1513 scanned, 11.7k on the 16-lane walk
    "pyramid_walk_per_query": (32, 512, "ground", [(1,), (2, (25.0, 0.0, 0.0)), (3, (3.0, -2.0, 0.0))],
                               {PYRAMID: 7000, SCAN16: 700, WALK16: 5000}),
    # 64 x 2048, batch 2, 30 m away: 2354 packets (packet walk), 7.9k queries on the 16-lane walk
    "packet_walk": (64, 2048, "ground", [(1, (30.0, 0.0, 0.0)), (2, (0.0, 30.0, 0.0))], {PACKET: 70000, WALK16: 4000}),
    # 272 x 2048: 272 super tiles, more than the pyramid keeps in registers -- no packets, the 315k queries without a usable bound
    # walk their (whole-image) bound windows tile by tile, one wave each (40 exposed); 2840 scanned (392 exposed), 16.4k on the
    # 16-lane walk (1589 exposed)
    "tile_walk_one_wave": (272, 2048, "ground", [(1, (0.5, 0.25, 0.0))], {WALK_WAVE: 150000, SCAN16: 1400, WALK16: 8000}),
    # the seam family: queries on y = 0 (the ground turned up by 90 degrees about x), targets mirrored in y; for x < 0 the two members
    # of a tie lie on either side of the azimuth seam.  64 x 512: 19.5k pyramid walks, 43 scans and 166 16-lane walks
    "seam_lists": (64, 512, "seam", [(1, (0.0, Z, 0.5), "x")], {PYRAMID: 9000, SCAN16: 20, WALK16: 80}),
    # 64 x 2048: 1243 packets, 78k queries on the packet walk
    "seam_packets": (64, 2048, "seam", [(1, (0.0, Z, 0.5), "x")], {PACKET: 40000}),
}


def _exact_batch(specs):
    return torch.stack([util.exact_pose(*s) for s in specs])


def _search_and_referee(H, W, family, T):
    sensor, tgt, src = tie_images(H, W, family)
    B = T.shape[0]
    tgt_b, src_b = tgt.expand(B, -1, -1, -1).contiguous(), src.expand(B, -1, -1, -1).contiguous()
    nn, match, tn, (counters, regime, a_idx, a_d2, window) = run_search(sensor, tgt_b, src_b, T)
    for b in range(B):
        check_match(nn[b], match[b], tgt_b[b], tn[b])
    stats = regime_stats(sensor, tgt_b, src_b, T, nn, regime, a_idx, a_d2)
    return sensor, tgt_b, src_b, nn, counters, regime, window, stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_nn_exact_ties_every_regime(name):
    """Zero mismatches against the float64 referee with the tie rule (smallest d2, then smallest pixel index), ``match`` a gather at
    the returned pixel, and the regime the case is about reached with at least the stated number of exact ties in it."""
    H, W, family, specs, floors = CASES[name]
    sensor, tgt_b, src_b, nn, counters, regime, window, stats = _search_and_referee(H, W, family, _exact_batch(specs))
    table = describe(stats, counters)
    print(f"{name}:\n{table}")
    for r, floor in floors.items():
        assert stats[r][1] >= floor, f"{name}: {stats[r][1]} exact ties in the {REGIME_NAMES[r]} regime, expected >= {floor}\n{table}"
    if WALK_WAVE in floors:       # whole-image bound windows, far beyond the seed-scan size
        assert int(((regime == WALK_WAVE) & (window > NN_SEED_MIN)).sum()) >= floors[WALK_WAVE], table
    if family == "seam":          # ties across the seam: a query behind the sensor (x < 0) answered in the image's first columns
        seam = 0
        for b in range(nn.shape[0]):
            sp, _, spix = util.lists_from_images(src_b[b], torch.zeros(3, H, W))
            Tb = util.exact_pose(*specs[b]).double()
            qx = Tb[0, :3] @ sp[0].double() + Tb[0, 3]
            got = nn[b][spix]
            seam += int(((qx < 0) & (got >= 0) & (got % W < W // 8)).sum())
        assert seam >= 100, f"{name}: only {seam} answers across the azimuth seam"
    bad = sum(s[3] for s in stats.values())
    util.measured(f"exact ties: {name}: queries that differ from the float64 referee", bad)
    assert bad == 0, f"{name}: {bad} queries differ from the float64 referee\n{table}"


def test_nn_exact_ties_windowed_packets():
    """64 x 512, batch 128, yaws of 0 / 90 / 180 / 270 degrees and small translations: each sample offers ~50 windowed packets, the batch
    6949 (more than NN_PACKET_WINDOWED), so pass B takes them -- 337k queries -- and 32k packets of queries without a bound go through
    the packet walk.  Every sample against the referee, zero mismatches (the unfixed kernel: 7962 scanned queries wrong)."""
    specs = [(k % 4, (0.125 * (k % 9), -0.0625 * (k % 7), 0.0)) for k in range(128)]
    _, _, _, _, counters, _, _, stats = _search_and_referee(64, 512, "ground", _exact_batch(specs))
    table = describe(stats, counters)
    print(table)
    assert counters[5] >= NN_PACKET_WINDOWED and counters[3] >= NN_PACKET_FEW, table
    assert stats[WPACKET][1] >= 20000 and stats[PACKET][1] >= 100000, table
    bad = sum(s[3] for s in stats.values())
    util.measured("exact ties: windowed packets: queries that differ from the float64 referee", bad)
    assert bad == 0, f"{bad} queries differ from the float64 referee\n{table}"


def _yaw(a, tx, ty):
    T = torch.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    T[0, 3], T[1, 3] = tx, ty
    return T


def _mirror_partner_pixels(tgt_img):
    """Pixel of the exact mirror image (z -> 2c - z) of every target pixel's point, -1 where the image does not hold it."""
    H, W = tgt_img.shape[-2:]
    tp, _, tpix = util.lists_from_images(tgt_img, torch.zeros(3, H, W))
    g = torch.round(tp[0].double() / util.GRID).long()
    assert g.abs().max() < 2 ** 16

    def key(x, y, z):
        return ((x + 2 ** 16) << 34) | ((y + 2 ** 16) << 17) | (z + 2 ** 16)
    k = key(g[0], g[1], g[2])
    order = torch.argsort(k)
    ks = k[order]
    km = key(g[0], g[1], round(2 * util.MIRROR_Z / util.GRID) - g[2])
    at = torch.searchsorted(ks, km).clamp(max=len(ks) - 1)
    hit = ks[at] == km
    partner = torch.full((H * W,), -1, dtype=torch.long)
    partner[tpix] = torch.where(hit, tpix[order[at]], torch.full_like(tpix, -1))
    return partner


def test_nn_ties_do_not_depend_on_the_batch():
    """A sample's correspondences do not depend on the rest of its batch.  64 x 512 under inexact yaws (q_z = c stays exact, so the
    mirror ties stay exact): alone, its packets are too few for the packet walk (per-query pyramid walks) and windowed packets do not
    exist; inside a batch of 128 whose other samples push the launch over NN_PACKET_FEW and NN_PACKET_WINDOWED, the same queries go
    through the packet walk and the windowed packets.  nn_pix and match must be bit-identical, and wherever the returned target's
    mirror partner is in the image, the returned pixel must be the lower of the two."""
    sensor, tgt, src = tie_images(64, 512, "ground")
    partner = _mirror_partner_pixels(tgt[0])
    fill = [util.exact_pose(k % 4, (0.125 * (k % 9), -0.0625 * (k % 7), 0.0)) for k in range(127)]
    HW = 64 * 512
    for yaw, tx, ty in ((0.37, 0.3, -0.2), (2.1, 1.2, 0.7), (-1.3, -0.9, 0.45)):
        T1 = _yaw(yaw, tx, ty).view(1, 4, 4)
        nn1, m1, _, (c1, reg1, _, _, _) = run_search(sensor, tgt, src, T1)
        TB = torch.cat([T1, torch.stack(fill)])
        B = TB.shape[0]
        nnB, mB, _, (cB, regB, _, _, _) = run_search(sensor, tgt.expand(B, -1, -1, -1).contiguous(), src.expand(B, -1, -1, -1).contiguous(), TB)
        assert c1[3] < NN_PACKET_FEW and cB[3] >= NN_PACKET_FEW and cB[5] >= NN_PACKET_WINDOWED, (c1, cB)
        moved = int((reg1 != regB[:HW]).sum())
        assert moved >= 1000 and int((regB[:HW] == WPACKET).sum()) > 0, f"only {moved} queries changed regime with the batch"
        assert torch.equal(nn1[0], nnB[0]) and torch.equal(m1[0], mB[0]), f"yaw {yaw}: {int((nn1[0] != nnB[0]).sum())} queries differ"
        got = nn1[0]
        has = (got >= 0) & (partner[got.clamp(min=0)] >= 0)
        pairs = int(has.sum())
        assert pairs >= 10000, f"only {pairs} answers with their mirror partner in the image"
        wrong = int((got[has] > partner[got[has]]).sum())
        assert wrong == 0, f"yaw {yaw}: {wrong} of {pairs} answers are the higher-index member of an exact tie"


def test_nn_bruteforce_kernel_tie_rule():
    """dl_nn_bruteforce (the referee of five search tests) returns the lowest list index of an exact tie: the lowest pixel index for
    raster-order lists.  Mirror scene at 64 x 512 under four exact poses, against the float64 referee; every query is a tie."""
    dev = _dev()
    sensor, tgt, src = tie_images(64, 512, "ground")
    tp, _, tpix = util.lists_from_images(tgt[0], torch.zeros(3, 64, 512))
    sp, _, _ = util.lists_from_images(src[0], torch.zeros(3, 64, 512))
    for spec in ((0,), (1, (0.5, -0.25, 0.0)), (2, (3.0, 1.0, 0.0)), (3, (-20.0, 7.5, 0.0))):
        T = util.exact_pose(*spec).double()
        q = T[:3, :3] @ sp[0].double() + T[:3, 3:]
        bf = _geo().nn_bruteforce(q.float().contiguous().to(dev), tp[0].to(dev)).cpu().long()
        ref, _, ties = util.nn_referee(q.to(dev), tp[0].to(dev), torch.arange(tp.shape[2]))
        assert int((ties >= 2).sum()) >= 0.9 * q.shape[1]
        assert torch.equal(bf, ref.cpu()), f"pose {spec}: {int((bf != ref.cpu()).sum())} differ"
        assert torch.equal(tpix[bf], tpix[ref.cpu()])
