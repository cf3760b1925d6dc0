"""tests/reproject_ref.py on the host: the reference of dl_reproject's contract is consistent with the reference of dl_project's, its
case generator meets the conditions the GPU tier (tests/test_gpu_reproject_exact.py) relies on -- every transformed point settled
within the allowed re-draws, the planted collisions present -- every defect of a list of plausible ones is told from the reference
by at least one generated case, and dl_reproject refuses bad arguments before any launch (the library loads without a GPU)."""
import ctypes

import numpy as np
import pytest

from tests import project_ref as pr
from tests import reproject_ref as rr

f32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype != f32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("moved4", "paired9", "src_pix"))


# ------------------------------------------------------------------------------------------------ the generator


def test_generator_settles_within_the_allowed_redraws_and_plants_what_it_promises():
    points = 0
    for name in rr.CASES:
        c = rr.case(name)
        assert rr.REDRAWS[name] <= rr.MAX_REDRAWS
        points += sum(q.shape[1] for q in c["ref"]["q"])
        ref, kinds = c["ref"], c["kinds"]
        for b, kind in enumerate(kinds):
            occ0, occ1 = ref["src_pix"][b, 0] >= 0, ref["src_pix"][b, 1] >= 0
            if kind in ("away", "nan"):
                assert not occ0.any() and not occ1.any() and not ref["moved4"][b].any() and not ref["paired9"][b].any(), (name, b)
                assert not np.signbit(ref["moved4"][b]).any() and not np.signbit(ref["paired9"][b]).any()
            else:
                assert occ0.any() and (occ1.any() or c["sen"].H * c["sen"].W < 256), (name, b)      # (a few dozen source pixels may hold no pair)
                assert not (occ1 & ~occ0).any()                       # a paired winner's pixel has a winner among all points
    print(f"[generator] re-draws per case: {rr.REDRAWS}; occupied transformed points in all cases: {points}")
    assert sum(rr.REDRAWS.values()) <= rr.MAX_REDRAWS                    # ~1e-7 per point: the reference alone stays far inside


def test_identity_returns_the_source_image_up_to_the_sign_of_zero():
    for name in ("min-identity", "odd-identity", "ragged-identity"):
        c = rr.case(name)
        src, got = c["src"][0], c["ref"]["moved4"][0]
        sp = c["ref"]["src_pix"][0, 0].reshape(-1)
        # planted twins and shadowed points lose their pixel; everywhere else a pixel keeps its own point
        own = sp == np.arange(sp.size)
        assert own.sum() >= 0.9 * (sp >= 0).sum()
        a, b = src.reshape(4, -1)[:, own], got.reshape(4, -1)[:, own]
        assert np.array_equal(a, b)                                       # values (-0.0 == +0.0)
        differ = _bits(a) != _bits(b)
        assert not differ.any() or (np.signbit(a[differ]).all() and not np.signbit(b[differ]).any() and (a[differ] == 0).all())


def test_planted_collisions_are_decided_as_the_contract_says():
    c = rr.case("ragged-rotation")
    ref = c["ref"]
    assert c["planted"]["shadowed"] == 1 and c["planted"]["duplicates"] == 1
    a, b = ref["src_pix"][0, 0], ref["src_pix"][0, 1]
    # somewhere a near unpaired point hides a far paired one: the two planes name different source pixels
    assert ((a >= 0) & (b >= 0) & (a != b)).any()
    # the twins: three source pixels with bit-equal points; the lowest of them is the only one that can appear
    src = c["src"][0].reshape(4, -1)
    _, inv, cnt = np.unique(_bits(src[:3]).T, axis=0, return_inverse=True, return_counts=True)
    twins = np.nonzero((cnt[inv.reshape(-1)] >= 3) & rr.occupied(*src[:3]))[0]
    assert len(twins) == 3
    assert not np.isin(twins[1:], a).any()


def test_reference_equals_project_ref_on_the_transformed_points():
    """moved4 is dl_project of the transformed source points in source-pixel order."""
    c = rr.case("ragged-large-B3")
    for b in range(c["B"]):
        q = c["ref"]["q"][b]
        img = pr.project([q], c["sen"], 3)["image4"][0]
        assert np.array_equal(_bits(img), _bits(c["ref"]["moved4"][b]))


# ------------------------------------------------------------------------------------------------ planted defects

DEFECTS = ("translation_before_rotation", "normal_translated", "residual_reversed", "key_range_of_the_source_point", "ties_to_higher_pixel",
           "pair_rule_or", "nn_pix_ignored", "occupancy_rule_of_normals", "round_half_away", "paired_winner_copied")


def _winners(u, v, r, idx, sen, defect):
    away = defect == "round_half_away"
    ru = (np.sign(u) * np.floor(np.abs(u) + f32(0.5))).astype(f32) if away else np.rint(u)
    rv = (np.sign(v) * np.floor(np.abs(v) + f32(0.5))).astype(f32) if away else np.rint(v)
    with np.errstate(invalid="ignore"):
        inside = (ru >= 0) & (ru <= sen.wm1f) & (rv >= 0) & (rv <= sen.hm1f)
    k = np.nonzero(inside)[0]
    pix = rv[k].astype(np.int64) * sen.W + ru[k].astype(np.int64)
    order = np.lexsort((-idx[k] if defect == "ties_to_higher_pixel" else idx[k], r[k].view(np.uint32), pix))
    ps = pix[order]
    first = np.ones(len(ps), dtype=bool)
    first[1:] = ps[1:] != ps[:-1]
    return k[order][first], ps[first]


def broken_reproject(c, defect):
    """A copy of reproject_ref.reproject_one with one defect switched on (None: the copy IS the reference)."""
    sen, B = c["sen"], c["B"]
    HW = sen.H * sen.W
    out = {"moved4": np.zeros((B, 4, HW), dtype=f32), "paired9": np.zeros((B, 9, HW), dtype=f32), "src_pix": np.full((B, 2, HW), -1, dtype=np.int32)}
    for b in range(B):
        src, srcn, match, nn, T = (c["src"][b].reshape(4, HW), c["srcn"][b].reshape(3, HW), c["match"][b].reshape(6, HW), c["nn"][b].reshape(HW),
                                   c["T"][b])
        if defect == "occupancy_rule_of_normals":
            occ_mask = (src[0] != 0) & (src[1] != 0) & (src[2] != 0)
        else:
            occ_mask = rr.occupied(src[0], src[1], src[2])
        occ = np.nonzero(occ_mask)[0]
        x, y, z = src[0, occ], src[1, occ], src[2, occ]
        with np.errstate(invalid="ignore", over="ignore"):
            if defect == "translation_before_rotation":
                q = np.stack(rr.rotate(T, x + T[0, 3], y + T[1, 3], z + T[2, 3]))
            else:
                q = np.stack(rr.transform(T, x, y, z))
        u, v, r = pr.coordinates(q, sen)
        key_r = pr.norm3(x, y, z) if defect == "key_range_of_the_source_point" else r
        win, pix = _winners(u, v, key_r, occ, sen, defect)
        out["moved4"][b][:3, pix], out["moved4"][b][3, pix], out["src_pix"][b][0, pix] = q[:, win], key_r[win], occ[win]    # (the stored range is the key's)
        hs, ht = rr.nonzero3(*srcn), rr.nonzero3(*match[3:6])
        pm = occ_mask & ((nn >= 0) | (defect == "nn_pix_ignored")) & ((hs | ht) if defect == "pair_rule_or" else (hs & ht))
        sel = np.nonzero(pm[occ])[0]
        if defect == "paired_winner_copied":
            keep = pm[occ[win]]
            wsel, ppix = win[keep], pix[keep]
        else:
            w, ppix = _winners(u[sel], v[sel], key_r[sel], occ[sel], sen, defect)
            wsel = sel[w]
        s = occ[wsel]
        with np.errstate(invalid="ignore", over="ignore"):
            out["paired9"][b][0:3, ppix] = q[:, wsel]
            if defect == "normal_translated":
                rn = np.stack(rr.transform(T, srcn[0, s], srcn[1, s], srcn[2, s]))
            else:
                rn = np.stack(rr.rotate(T, srcn[0, s], srcn[1, s], srcn[2, s]))
            out["paired9"][b][3:6, ppix] = rn
            d = (match[0:3, s] - q[:, wsel]) if defect == "residual_reversed" else (q[:, wsel] - match[0:3, s])
            out["paired9"][b][6:9, ppix] = d.astype(f32)
        out["src_pix"][b][1, ppix] = s
    H, W = sen.H, sen.W
    return {"moved4": out["moved4"].reshape(B, 4, H, W), "paired9": out["paired9"].reshape(B, 9, H, W), "src_pix": out["src_pix"].reshape(B, 2, H, W)}


def test_every_planted_defect_is_told_from_the_reference():
    caught = {d: [] for d in DEFECTS}
    for name in rr.CASES:
        c = rr.case(name)
        assert _same(broken_reproject(c, None), c["ref"]), name           # without a defect the copy IS the reference
        for d in DEFECTS:
            if not _same(broken_reproject(c, d), c["ref"]):
                caught[d].append(name)
    for d in DEFECTS:
        print(f"[defects] {d}: told apart by {len(caught[d])} cases, e.g. {caught[d][:4]}")
        assert caught[d], f"no generated case tells the defect '{d}' from the reference"


# ------------------------------------------------------------------------------------------------ the entry point, without a GPU


def test_workspace_bytes_are_the_two_key_planes():
    from delora_amd import _lib
    lib = _lib.load()
    for B, H, W in ((1, 2, 2), (3, 5, 9), (1, 5, 9), (1, 64, 2048), (8, 64, 720), (3, 16, 130)):
        assert lib.dl_reproject_workspace_bytes(B, H, W) == (B * 2 * H * W * 8 + 15) // 16 * 16
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -3)):
        assert lib.dl_reproject_workspace_bytes(*bad) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """No device is touched before the checks: fake non-null pointers are enough, on a machine without a GPU too."""
    from delora_amd import _lib
    lib = _lib.load()
    sen = _lib.SensorStruct(16, 130, -3.1, 3.1, -0.4, 0.03)
    HW = 16 * 130
    P, N = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def call(src=P, src_ss=4 * HW, srcn=P, srcn_ss=3 * HW, match=P, match_ss=6 * HW, nn=P, T=P, B=1, sensor=sen, moved4=P, paired9=P,
             src_pix=P, ws=P):
        return lib.dl_reproject(src, src_ss, srcn, srcn_ss, match, match_ss, nn, T, B, ctypes.byref(sensor) if sensor is not None else None,
                                moved4, paired9, src_pix, ws, N)

    refusals = [({"src": N}, b"null pointer"), ({"T": N}, b"null pointer"), ({"moved4": N}, b"null pointer"), ({"ws": N}, b"null pointer"),
                ({"sensor": None}, b"null pointer"), ({"B": 0}, b"B=0"), ({"B": -2}, b"B=-2"),
                ({"sensor": _lib.SensorStruct(1, 130, -3.1, 3.1, -0.4, 0.03)}, b"H=1"), ({"sensor": _lib.SensorStruct(16, 1, -3.1, 3.1, -0.4, 0.03)}, b"W=1"),
                ({"B": 1 << 20}, b"exceed"),
                ({"srcn": N}, b"only together"), ({"match": N}, b"only together"), ({"nn": N}, b"only together"),
                ({"srcn": N, "match": N, "nn": N}, b"paired9 needs"),
                ({"src_ss": 3 * HW - 1}, b"src_ss=6239"), ({"srcn_ss": 3 * HW - 1}, b"srcn_ss=6239"), ({"match_ss": 6 * HW - 1}, b"match_ss=12479"),
                ({"ws": ctypes.c_void_p(4096 + 8)}, b"16-byte aligned")]
    for kw, text in refusals:
        assert call(**kw) == -1, kw
        assert text in lib.dl_last_error(), (kw, lib.dl_last_error())
