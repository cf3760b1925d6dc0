"""tests/project_ref.py on the host: the reference of the projection contract agrees with the torch-CPU oracle and the goldens outside
the atan2 ambiguity mask, its correctly rounded fp32 steps equal rational arithmetic, its generators meet the conditions the GPU
tier (tests/test_gpu_project_exact.py) relies on, every defect of a list of plausible ones is told from the reference by at least
one generated case -- and dl_project refuses bad arguments before any launch (the library loads without a GPU)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import project_ref as pr
from tests import util
from tests.util import orc

f32 = np.float32


def _pixels(u, v, sen):
    ru, rv = np.rint(u), np.rint(v)
    with np.errstate(invalid="ignore"):
        inside = (ru >= 0) & (ru <= sen.wm1f) & (rv >= 0) & (rv <= sen.hm1f)
    pix = np.full(len(u), -1, dtype=np.int64)
    pix[inside] = rv[inside].astype(np.int64) * sen.W + ru[inside].astype(np.int64)
    return pix


def _bits(a):
    """uint32 view with every NaN mapped to one pattern (which NaN an operation produces is the platform's choice)."""
    a = np.ascontiguousarray(a, dtype=f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


# ------------------------------------------------------------------------------------------------ reference vs oracle and goldens


@pytest.mark.parametrize("name", list(pr.SENSOR_TABLE))
def test_reference_equals_the_oracle_outside_the_ambiguity_mask(name):
    sen = pr.sensor(name)
    o = util.oracle_sensor(sen.H, sen.W, sen.vfov, sen.hfov)
    p = np.array(pr.coordinate_points(name))
    opix, ou, ov = util.reference_pixels(p, o)
    u, v, r = pr.coordinates(p, sen)
    differ = _pixels(u, v, sen) != opix
    assert not np.any(differ & ~util.ambiguity_mask(p, o)), "pixel differs outside the ambiguity mask"
    fin = np.isfinite(p).all(axis=0)
    assert np.nanmax(np.abs(u[fin] - ou[fin])) < 2e-3 and np.nanmax(np.abs(v[fin] - ov[fin])) < 2e-3
    orange = torch.norm(torch.from_numpy(p), dim=0).numpy()
    big = np.abs(p).max(axis=0) >= 1e19
    assert np.array_equal(_bits(r[~big]), _bits(orange[~big])), "range differs from torch.norm"     # (torch rescales huge vectors)
    # the whole image of a plain cloud, away from pixels an ambiguous point may or may not land in
    scan = pr.with_aux(pr.random_mix(3000, 77), 5, 3)
    ref = pr.project([scan], sen, 5)
    img, _, _, idx, pix = orc.project_to_img(torch.from_numpy(scan)[None], o)
    clean = ~util.tainted_pixels(scan, o)
    img = img[0].numpy()
    assert np.array_equal(ref["image4"][0][:, clean], np.concatenate([img[:3], img[5:6]])[:, clean])
    assert np.array_equal(ref["aux"][0][:, clean], img[3:5][:, clean])
    exp_map = -np.ones((sen.H, sen.W), dtype=np.int64)
    exp_map[pix[0, :, 0].numpy(), pix[0, :, 1].numpy()] = idx.numpy()
    assert np.array_equal(ref["pix2pt"][0][clean], exp_map[clean])
    assert np.array_equal(ref["packed"][0][..., 3], ref["image4"][0][3]) and not ref["packed_aux"][0][..., 2:].any()


@pytest.mark.parametrize("name", ["small", "small_c6", "mid", "edge", "all_outside"])
def test_reference_replays_the_projection_goldens(name):
    g = util.load_golden("proj_" + name)
    sen = pr.sensor_constants(int(g["H"]), int(g["W"]), [float(x) for x in g["vfov"]], [float(x) for x in g["hfov"]])
    o = util.oracle_sensor(g["H"], g["W"], g["vfov"], g["hfov"])
    scan = g["scan"].astype(f32)
    C = scan.shape[0]
    ref = pr.project([scan], sen, C)
    clean = ~util.tainted_pixels(scan, o)
    exp_map = -np.ones((sen.H, sen.W), dtype=np.int64)
    exp_map[g["pix"][0][:, 0], g["pix"][0][:, 1]] = g["idx"]
    rng = ref["uvr"][2]
    bad = np.argwhere((ref["pix2pt"][0] != exp_map) & clean)
    for r, c in bad:       # the reference's argsort is not stable: two points of one pixel with bit-equal range are a legitimate tie
        a, b = int(ref["pix2pt"][0][r, c]), int(exp_map[r, c])
        assert a >= 0 and b >= 0 and rng[a] == rng[b] and a < b, (r, c, a, b)
    assert len(bad) <= 4
    tie = np.zeros_like(clean)
    tie[tuple(bad.T)] = True
    gi = g["image"][0]
    ok = clean & ~tie
    assert np.array_equal(ref["image4"][0][:, ok], np.concatenate([gi[:3], gi[C:C + 1]])[:, ok])
    if C > 3:
        assert np.array_equal(ref["aux"][0][:, ok], gi[3:C][:, ok])


def test_sensor_constants_form_the_span_in_fp64():
    s = pr.sensor("kitti")
    assert s.hspanf == f32(359.8 * pr.DEG) or s.hspanf == f32(179.9 * pr.DEG - -179.9 * pr.DEG)
    assert s.hf0f == f32(-179.9 * pr.DEG) and s.wm1f == f32(719) and s.hm1f == f32(63)
    assert s.vspanf == f32(2.0 * pr.DEG - -24.5 * pr.DEG)
    f = pr.sensor("flipped")
    assert f.hspanf < 0 and f.vspanf < 0


# ------------------------------------------------------------------------------------------------ correctly rounded steps


def _frac(x):
    return Fraction(float(x))


def test_round_fraction_to_f32_edges():
    R = pr.round_fraction_to_f32
    one, eps = Fraction(1), Fraction(2) ** -23
    assert R(one + eps / 2) == f32(1.0) and R(one + 3 * eps / 2) == f32(1.0) + f32(2.0 ** -22)       # ties to even
    assert R(one + eps / 2 + Fraction(2) ** -80) == f32(1.0 + 2.0 ** -23)
    assert R(Fraction(2) ** -150) == f32(0.0) and R(Fraction(2) ** -150 + Fraction(2) ** -200) == f32(2.0 ** -149)
    assert R(3 * Fraction(2) ** -150) == f32(2.0 ** -148)                                             # subnormal tie to even
    top = (2 - Fraction(2) ** -23) * Fraction(2) ** 127
    assert R(top) == np.finfo(f32).max and R(top + Fraction(2) ** 103) == f32(np.inf) and R(top + Fraction(2) ** 103 - 1) == np.finfo(f32).max
    assert R(-top - Fraction(2) ** 103) == f32(-np.inf)
    rng = np.random.default_rng(1)
    x = rng.normal(size=300) * 10.0 ** rng.uniform(-44, 38, 300)
    with np.errstate(over="ignore"):
        assert all(R(Fraction(float(t))) == f32(t) for t in x)                                        # numpy's own fp64 -> fp32 rounding


def test_fma32_and_sqrt32_equal_rational_arithmetic():
    # the planted double-rounding case: a*b = 2^-24 - 2^-64, c = 1 + 2^-23: the fp64 sum is the midpoint 1 + 2^-23 + 2^-24
    a, b, c = f32(2.0 ** -12 * (1 + 2.0 ** -20)), f32(2.0 ** -12 * (1 - 2.0 ** -20)), f32(1 + 2.0 ** -23)
    naive = f32(np.float64(a) * np.float64(b) + np.float64(c))
    assert naive == f32(1 + 2.0 ** -22), "the naive evaluation rounds twice here"
    assert pr.fma32(a, b, c)[0] == f32(1 + 2.0 ** -23) == pr.round_fraction_to_f32(_frac(a) * _frac(b) + _frac(c))
    rng = np.random.default_rng(2)
    n = 1500
    x = (rng.normal(size=(3, n)) * 10.0 ** rng.uniform(-24, 19.4, (3, n))).astype(f32)
    x[:, :200] = np.round(x[:, :200] / np.abs(x[:, :200]).max(axis=0) * 4096) .astype(f32)           # short mantissas: exact sums, ties
    x[:, 200:260] = (rng.normal(size=(3, 60)) * 1e-21).astype(f32)                                     # squares in the subnormals
    got = pr.fma32(x[0], x[1], x[2])
    for i in range(n):
        assert got[i] == pr.round_fraction_to_f32(_frac(x[0, i]) * _frac(x[1, i]) + _frac(x[2, i])), x[:, i]
    sq = pr.fma32(x[1], x[1], pr.mul32(x[0], x[0]))
    for i in range(n):
        xx = pr.round_fraction_to_f32(_frac(x[0, i]) ** 2)
        if np.isinf(xx):                                           # the square overflowed: the sum stays +inf
            assert sq[i] == f32(np.inf)
            continue
        assert sq[i] == pr.round_fraction_to_f32(_frac(x[1, i]) ** 2 + _frac(xx))
    # sqrt: r is the correctly rounded root of a iff a lies strictly between the squares of r's two rounding midpoints
    a = np.abs(x.reshape(-1)[:2000])
    a = a[(a > 1e-30) & np.isfinite(a)]
    r = pr.sqrt32(a)
    for ai, ri in zip(a, r):
        lo = (_frac(ri) + _frac(np.nextafter(ri, f32(0)))) / 2
        hi = (_frac(ri) + _frac(np.nextafter(ri, f32(np.inf)))) / 2
        assert lo * lo <= _frac(ai) <= hi * hi, (ai, ri)
    assert pr.norm3(f32([3e38, 1e20, 0]), f32([0, 1e20, 0]), f32([0, 0, 0])).tolist() == [np.inf, np.inf, 0.0]
    assert pr.norm3(f32([3.0]), f32([4.0]), f32([12.0]))[0] == f32(13.0)


def test_settled_is_arbitrated_by_a_high_precision_atan2():
    """Where ``settled`` says yes, the float32 nearest to the TRUE angle (mpmath, 100 digits) is the reference's; the distance it
    reports is the true distance to the midpoint up to the libm's own error."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 200
    p = np.concatenate([pr.random_mix(700, 9), np.array(pr.exact_halves(pr.sensor("kitti"))[0][:, :100])], axis=1)
    assert pr.settled(p).all()
    a64, e64 = pr._angles64(p)
    n2 = pr.norm2(p[0], p[1])
    for i in range(p.shape[1]):
        for got, yy, xx in ((a64[i], p[1, i], p[0, i]), (e64[i], p[2, i], n2[i])):
            true = mpmath.atan2(mpmath.mpf(float(yy)), mpmath.mpf(float(xx)))
            assert abs(true - mpmath.mpf(float(got))) <= 1.0 * float(np.spacing(abs(got))), "libm atan2 off by more than 1 ulp"
            lo, hi = sorted((float(f32(got)), float(np.nextafter(f32(got), f32(np.inf) if float(f32(got)) < true else f32(-np.inf)))))
            nearest = lo if true - lo < hi - true else hi
            assert nearest == float(f32(got))
    # a value planted 3 ulp64 from a midpoint is not settled
    mid = 0.5 * (np.float64(f32(0.7)) + np.float64(np.nextafter(f32(0.7), f32(1))))
    near = mid + 3 * np.spacing(mid)
    assert pr.midpoint_distance_ulps(np.array([near]))[0] == 3.0 and pr.midpoint_distance_ulps(np.array([0.7]))[0] > 1e6


# ------------------------------------------------------------------------------------------------ generator conditions


def test_generators_meet_their_conditions():
    pr.REPLACED.clear()
    counts = {}
    for name in pr.SENSOR_TABLE:
        sen = pr.sensor(name)
        pr.coordinate_points.cache_clear()
        before = {k: v for k, v in pr.REPLACED.items()}
        p = pr.coordinate_points(name)
        fin = np.isfinite(p).all(axis=0)
        assert pr.settled(p[:, fin]).all()
        xh, ku, kv = pr.exact_halves(sen)
        u, v, _ = pr.coordinates(xh, sen)
        assert np.all(u[ku >= 0] == (ku[ku >= 0] + 0.5).astype(f32)) and np.all(v[kv >= 0] == (kv[kv >= 0] + 0.5).astype(f32))
        eu, ou = len(set(ku[(ku >= 0) & (ku % 2 == 0)])), len(set(ku[(ku >= 0) & (ku % 2 == 1)]))
        ev, ov = len(set(kv[(kv >= 0) & (kv % 2 == 0)])), len(set(kv[(kv >= 0) & (kv % 2 == 1)]))
        replaced = sum(pr.REPLACED[k][0] - before.get(k, (0, 0))[0] for k in pr.REPLACED)
        counts[name] = (eu, ou, ev, ov, replaced, p.shape[1])
        print(f"[generators] {name}: {p.shape[1]} points, exact halves u even/odd {eu}/{ou}, v even/odd {ev}/{ov}, replaced as unsettled {replaced}")
        if name in pr.DATASET_SENSORS:
            assert eu >= 8 and ou >= 8 and ev >= 4 and ov >= 4, (name, eu, ou, ev, ov)
        assert replaced <= 1e-5 * p.shape[1]
        # specials: signed zeros, subnormals, overflow, NaN and inf are all there; the aux channels stay finite
        sp = pr.specials(sen)
        assert np.isnan(sp).any(axis=1).all() and np.isinf(sp).any(axis=1).all() and (np.abs(sp) >= 1e19).any()
        assert (np.signbit(sp) & (sp == 0)).any(axis=1).all() and ((np.abs(sp) > 0) & (np.abs(sp) < 1.1e-38)).any()
        assert np.isfinite(pr.with_aux(sp, 8, 1)[3:]).all()
        us, vs, rs = pr.coordinates(sp, sen)
        assert np.isinf(rs).any() and (rs == 0).any()
        if abs(sen.hfov[0]) < np.pi - 1e-3 and sen.W <= 1800:       # the field of view ends before the seam: both overhangs exist
            assert ((us >= -0.5) & (us < 0)).any() and ((us > sen.wm1f) & (us <= sen.wm1f + f32(0.5))).any(), name
            assert (np.signbit(np.rint(us)) & (np.rint(us) == 0)).any()
        if abs(sen.vfov[0]) < np.pi / 2 - 1e-3:
            assert ((vs >= -0.5) & (vs < 0)).any() and ((vs > sen.hm1f) & (vs <= sen.hm1f + f32(0.5))).any(), name
    for k, (done, total) in pr.REPLACED.items():
        print(f"[generators] {k}: {done} of {total} points replaced as unsettled")
        assert done <= 1e-5 * total
    # ties: at least 4 points of bit-equal range in every group of the coarse sensor (duplicates only make them larger)
    tc = pr.tie_cloud()
    groups = pr.tie_groups(tc[:, np.abs(tc).max(axis=0) < 1e19], pr.sensor("coarse"))
    print(f"[generators] tie_cloud: {tc.shape[1]} points, {len(groups)} (pixel, range) groups on coarse, sizes {groups.min()}..{groups.max()}")
    assert len(groups) >= 100 and groups.min() >= pr.TIE_MIN_GROUP
    assert np.unique(tc, axis=1).shape[1] < tc.shape[1]                                           # exact duplicates
    for sname in ("coarse", "ragged"):
        sen = pr.sensor(sname)
        ref = pr.project([tc], sen, 3)
        u, v, r = pr.coordinates(tc, sen)
        pix = _pixels(u, v, sen)
        far = np.isinf(r) & (pix >= 0)
        won = ref["pix2pt"][0].reshape(-1)
        lost = [i for i in np.nonzero(far)[0] if won[pix[i]] != i and np.isfinite(r[won[pix[i]]])]
        alone = [i for i in np.nonzero(far)[0] if won[pix[i]] == i]
        assert lost, "no inf-range point shares a pixel with a finite one"
        if sname == "ragged":
            assert alone, "no inf-range point wins a pixel"
            assert all(np.isinf(r[pix == pix[i]]).all() for i in alone)
    # the cap scans: raster order, a second trip of the vote's loop that matters
    big = pr.cap_scans(1)[0]
    assert big.shape[1] == pr.CAP_POINTS > 1024 * 256
    ref = pr.project([big], pr.sensor("kitti"), 3)
    assert int((ref["pix2pt"] >= 1024 * 256).sum()) >= 250
    pix = _pixels(*pr.coordinates(big, pr.sensor("kitti"))[:2], pr.sensor("kitti"))[:1024 * 256]
    assert np.mean(np.abs(np.diff(pix)) <= 2) > 0.9, "not in raster order"
    # the layout cases: every S, every C, each optional output given and left out, G = 12 where S % 8 != 0
    cases = pr.layout_cases()
    assert {len(c["lens"]) for c in cases} == set(pr.LAYOUT_S) and {c["C"] for c in cases} == set(pr.LAYOUT_C)
    for opt in ("packed", "packed_aux", "kept", "uvr"):
        assert any(opt in c["null"] for c in cases) and any(opt not in c["null"] and (opt != "packed_aux" or c["C"] >= 6) for c in cases)
    for S in (9, 17):
        assert any(len(c["lens"]) == S and max(c["lens"]) == 3000 for c in cases)
    assert any(max(c["lens"]) == 0 for c in cases) and any(c["skew"] == 16 for c in cases)
    assert any(len(c["lens"]) % 2 == 1 and c["sensor"] == "odd" for c in cases)


# ------------------------------------------------------------------------------------------------ the suite can fail

DEFECTS = ("ties_to_higher_index", "floor_half_up", "lt_at_last_column", "lt_at_last_row", "negative_zero_outside", "range_truncated_bits",
           "aux_from_neighbour", "zero_fill_one_channel_early", "ghost_group_last_scan_skipped", "second_trip_skipped", "span_of_fp32_ends")


def broken_project(scans, sen, C, coords, defect):
    """A copy of project_ref.project / winners with one defect switched on."""
    S, H, W = len(scans), sen.H, sen.W
    out = {"image4": np.zeros((S, 4, H * W), dtype=f32), "aux": np.zeros((S, max(C - 3, 0), H * W), dtype=f32),
           "packed_aux": np.zeros((S, H * W, 4), dtype=f32), "pix2pt": np.full((S, H * W), -1, dtype=np.int32)}
    for s, scan in enumerate(scans):
        if defect == "ghost_group_last_scan_skipped" and S >= 8 and S % 8 and s == S - 1:
            continue
        u, v, r = coords[s]
        n = len(u)
        ru, rv = (np.floor(u + f32(0.5)), np.floor(v + f32(0.5))) if defect == "floor_half_up" else (np.rint(u), np.rint(v))
        with np.errstate(invalid="ignore"):
            in_u = (ru >= 0) & ((ru < sen.wm1f) if defect == "lt_at_last_column" else (ru <= sen.wm1f))
            in_v = (rv >= 0) & ((rv < sen.hm1f) if defect == "lt_at_last_row" else (rv <= sen.hm1f))
        inside = in_u & in_v
        if defect == "negative_zero_outside":
            inside &= ~np.signbit(ru) & ~np.signbit(rv)
        if defect == "second_trip_skipped":
            inside &= np.arange(n) < 1024 * 256
        idx = np.nonzero(inside)[0]
        pix = rv[idx].astype(np.int64) * W + ru[idx].astype(np.int64)
        rb = r[idx].view(np.uint32)
        if defect == "range_truncated_bits":
            rb = rb >> 8
        order = np.lexsort((-idx if defect == "ties_to_higher_index" else idx, rb, pix))
        ps = pix[order]
        first = np.ones(len(ps), dtype=bool)
        first[1:] = ps[1:] != ps[:-1]
        win, pix = idx[order][first], ps[first]
        src = np.minimum(win + 1, n - 1) if defect == "aux_from_neighbour" else win
        out["image4"][s, :3, pix], out["image4"][s, 3, pix] = scan[:3, win].T, r[win]
        for c in range(3, C):
            val = scan[c, src]
            if defect == "zero_fill_one_channel_early" and c == 4 and C <= 5:
                val = np.zeros_like(val)
            out["aux"][s, c - 3, pix] = val
            if c < 6:
                out["packed_aux"][s, pix, c - 3] = val
        out["pix2pt"][s, pix] = win
    out["uvr"] = np.concatenate([np.stack(c) for c in coords], axis=1)
    return out


def _generated_cases():
    """(name, sensor, scans, C) of everything the GPU tier runs."""
    for name in pr.SENSOR_TABLE:
        yield "coords/" + name, pr.sensor(name), [np.array(pr.coordinate_points(name))], 3
    tc = pr.tie_cloud()
    for sname in ("coarse", "ragged"):
        for perm in (0, 1):
            yield f"ties/{sname}/perm{perm}", pr.sensor(sname), [tc if perm == 0 else np.ascontiguousarray(tc[:, ::-1])], 3
    for c in pr.layout_cases():
        yield "layout/" + c["name"], pr.sensor(c["sensor"]), pr.case_scans(c), c["C"]
    for S in (1, 8):
        yield f"cap/S{S}", pr.sensor("kitti"), list(pr.cap_scans(S)), 3


def _same(got, ref):
    """A broken_project result equals the reference's in every output it builds (bit patterns; any NaN equals any NaN)."""
    for k, g in got.items():
        r = ref[k].reshape(g.shape)
        if not np.array_equal(_bits(g), _bits(r)) if g.dtype == f32 else not np.array_equal(g, r):
            return False
    return True


def _scans_in(case_name):
    return int(case_name.split("-S")[1].split("-")[0])


def test_every_planted_defect_is_told_from_the_reference():
    caught = {d: [] for d in DEFECTS}
    for name, sen, scans, C in _generated_cases():
        coords = [pr.coordinates(s[:3], sen) for s in scans]
        ref = pr.project(scans, sen, C, coords)
        if name == "coords/kitti":         # without a defect the copy IS the reference: the comparison below is not vacuous
            assert _same(broken_project(scans, sen, C, coords, None), ref)
        for d in DEFECTS:
            if d == "span_of_fp32_ends":
                if not name.startswith("coords/"):
                    continue
                bad = pr.sensor_constants(sen.H, sen.W, sen.vfov, sen.hfov)
                bad.hspanf, bad.vspanf = f32(sen.hfov[1]) - f32(sen.hfov[0]), f32(sen.vfov[1]) - f32(sen.vfov[0])
                got = broken_project(scans, sen, C, [pr.coordinates(s[:3], bad) for s in scans], d)
            else:
                got = broken_project(scans, sen, C, coords, d)
            if not _same(got, ref):
                caught[d].append(name)
    for d in DEFECTS:
        print(f"[defects] {d}: told apart by {len(caught[d])} cases, e.g. {caught[d][:4]}")
        assert caught[d], f"no generated case tells the defect '{d}' from the reference"
    every, shipped = {"coords/" + s for s in pr.SENSOR_TABLE}, {"coords/" + s for s in pr.DATASET_SENSORS}
    assert any(n.startswith("ties/") for n in caught["ties_to_higher_index"])
    assert set(caught["floor_half_up"]) >= shipped
    assert set(caught["lt_at_last_column"]) >= every and set(caught["lt_at_last_row"]) >= every
    assert {"coords/kitti", "coords/flipped"} <= set(caught["negative_zero_outside"])
    assert all(_scans_in(n) >= 8 and _scans_in(n) % 8 for n in caught["ghost_group_last_scan_skipped"])
    assert set(caught["second_trip_skipped"]) == {"cap/S1", "cap/S8"}
    assert all("-C5" in n for n in caught["zero_fill_one_channel_early"])
    # at every sensor of the table but "span" the two ways of forming the span give the same fp32 number
    assert caught["span_of_fp32_ends"] == ["coords/span"]
    s = pr.sensor("span")
    assert f32(s.vfov[1]) - f32(s.vfov[0]) != s.vspanf


# ------------------------------------------------------------------------------------------------ refusals


def test_dl_project_refuses_bad_arguments_before_any_launch():
    """Host memory stands in for every pointer: a call that got as far as a launch would not return DL_ERR_INVALID_ARGUMENT."""
    from delora_amd import _lib
    lib = _lib.load()
    raw = (ctypes.c_float * 256)()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    P = ctypes.c_void_p(base)
    sen = _lib.SensorStruct(16, 130, -3.1, 3.1, -0.4, 0.03)

    def call(**kw):
        a = dict(pts=P, pts_cs=100, n_cols=100, offs=P, S=1, C=3, max_n=100, sensor=ctypes.byref(sen), image4=P, aux=None, packed=None,
                 packed_aux=None, pix2pt=P, workspace=P, kept=None, uvr=None)
        a.update(kw)
        return lib.dl_project(a["pts"], a["pts_cs"], a["n_cols"], a["offs"], a["S"], a["C"], a["max_n"], a["sensor"], a["image4"], a["aux"],
                              a["packed"], a["packed_aux"], a["pix2pt"], a["workspace"], a["kept"], a["uvr"], None)

    def refused(text, **kw):
        rc = call(**kw)
        err = lib.dl_last_error()
        assert rc == -1 and b"dl_project" in err and text in err, (kw, rc, err)

    for k in ("pts", "offs", "image4", "pix2pt", "workspace"):
        refused(b"null pointer", **{k: None})
    refused(b"null pointer", sensor=None)
    for kw in (dict(S=0), dict(S=-1), dict(C=2), dict(max_n=-1), dict(n_cols=-1), dict(n_cols=101), dict(n_cols=8, pts_cs=7)):
        refused(b"bad sizes", **kw)
    for H, W in ((1, 130), (16, 1), (0, 0)):
        refused(b"bad sizes", sensor=ctypes.byref(_lib.SensorStruct(H, W, -3.1, 3.1, -0.4, 0.03)))
    refused(b"n_cols=101 pts_cs=100", n_cols=101)
    for C in (4, 6, 8):
        refused(b"needs an aux image", C=C, aux=None)
    for C in (3, 4, 5):
        refused(b"packed_aux needs C >= 6", C=C, aux=P, packed_aux=P)
    for off in (4, 8, 12):
        refused(b"workspace must be 16-byte aligned", workspace=ctypes.c_void_p(base + off))
        refused(b"workspace must be 16-byte aligned", workspace=ctypes.c_void_p(base + off), C=6, aux=P, packed_aux=P, kept=P, uvr=P)
    assert lib.dl_project_workspace_bytes(3, 5, 9, 0, 3) == 3 * 45 * 8 + 8, "an odd key plane is padded to 16 bytes"
    assert lib.dl_project_workspace_bytes(3, 5, 9, 11, 3) == 3 * 45 * 8 + 8 + 11 * 16 and lib.dl_project_workspace_bytes(3, 5, 9, 11, 4) == 3 * 45 * 8 + 8 + 11 * 32
    for bad in ((0, 5, 9, 1, 3), (1, 0, 9, 1, 3), (1, 5, 0, 1, 3), (1, 5, 9, -1, 3), (1, 5, 9, 1, 2)):
        assert lib.dl_project_workspace_bytes(*bad) == 0
