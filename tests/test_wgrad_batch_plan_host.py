"""Host side of the four merged weight-gradient entry points (csrc/wgrad_batch.h and its callers in conv.hip, wgradh.hip, wino.hip):
workspace bytes, return codes, error texts and the plan text -- kernel instantiation, grid and the ``slabs=`` notes in launch order -- of
a fixed set of layer tables, as ``tools/bin/wgrad_plan_dump`` prints them, against ``tests/golden/wgrad_batch_plans.json``.  The golden
file was recorded with the same program on the commit BEFORE the host side moved into the shared helper
(``python -m tests.test_wgrad_batch_plan_host --record``); nothing in it may change without a change of what runs on the GPU.  No GPU.
"""
import json
import os
import subprocess
import sys

import pytest

from delora_amd import _lib
from delora_amd.models import ring_conv as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, "tools", "bin", "wgrad_plan_dump")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_batch_plans.json")
BATCH = _lib.WGRAD_BATCH


def trunk_layers(B, H, W):
    """(N, H, W, C, K, ksize, stride_h, stride_w) of the 19 trunk convolutions behind the stem of an H x W image (stem and pooling
    halve the width twice), in the order the backward pass collects them (last layer first)."""
    w1 = rc.out_size(rc.out_size(W, 2), 2)
    w2, w3 = rc.out_size(w1, 2), rc.out_size(rc.out_size(w1, 2), 2)
    w4, h4 = rc.out_size(w3, 2), rc.out_size(H, 2)
    fwd = [(B, H, w1, 64, 64, 3, 1, 1)] * 4
    fwd += [(B, H, w1, 64, 128, 3, 1, 2), (B, H, w1, 64, 128, 1, 1, 2)] + [(B, H, w2, 128, 128, 3, 1, 1)] * 3
    fwd += [(B, H, w2, 128, 256, 3, 1, 2), (B, H, w2, 128, 256, 1, 1, 2)] + [(B, H, w3, 256, 256, 3, 1, 1)] * 3
    fwd += [(B, H, w3, 256, 512, 3, 2, 2), (B, H, w3, 256, 512, 1, 2, 2)] + [(B, h4, w4, 512, 512, 3, 1, 1)] * 3
    return fwd[::-1]


def trunk_family(layers, family):
    """The layers of a trunk that ``ring_conv.wgrad_batch`` hands to ``family`` (its rules, restated on shapes)."""
    out = []
    for (N, H, W, C, K, ks, sh, sw) in layers:
        if ks == 3 and (sh, sw) == (1, 1) and C >= rc.WINO_WGRAD_MIN_C_BATCHED:
            fam = "wino"
        elif ks == 3 and rc.wino_strided_wgrad_ok(N, H, W, C, K, (sh, sw)) and N * (H // 2) * (W // 32) >= rc.WINO_STRIDED_WGRAD_MIN_CHUNKS:
            fam = "pair"
        else:
            fam = "direct"
        if fam == family:
            out.append((N, H, W, C, K, ks, sh, sw))
    return out


def _s1(shapes):
    return [s + (3, 1, 1) for s in shapes]


def _s12(shapes):
    return [s + (3, 1, 2) for s in shapes]


# the tables of tests/test_gpu_wgrad_batch_digest.py: the first layer of each is one chunk (one slab, written in place), the rest split
DIGEST = {
    "direct": [(1, 1, 32, 64, 64, 3, 1, 1), (2, 8, 32, 128, 64, 3, 1, 1), (1, 7, 30, 64, 64, 3, 1, 1), (2, 8, 64, 64, 128, 3, 1, 2),
               (2, 8, 64, 128, 128, 1, 2, 2), (8, 16, 64, 64, 64, 3, 1, 1)],
    "wino": _s1([(1, 2, 16, 128, 64), (2, 8, 32, 128, 64), (1, 31, 7, 128, 128), (1, 7, 30, 64, 64), (8, 16, 64, 64, 64)]),
    "half": [(1, 2, 32, 64, 64, 3, 1, 1), (2, 8, 64, 128, 128, 3, 1, 1), (2, 8, 32, 64, 64, 3, 1, 1), (2, 8, 64, 64, 128, 3, 1, 2),
             (1, 7, 30, 128, 64, 3, 1, 1)],
    "pair": _s12([(1, 2, 32, 64, 64), (2, 8, 64, 64, 128), (1, 4, 128, 128, 64)]),
}
DTYPES = {"direct": ("f32",), "wino": ("f32",), "pair": ("f32",), "half": ("bf16", "f16")}

# one layer / DL_WGRAD_BATCH layers / at least two launch groups / a one-chunk layer beside large ones / three refused tables
_BIG = {
    "direct": [(8, 64, 512, 64, 64, 3, 1, 1), (8, 64, 256, 128, 128, 3, 1, 1), (4, 64, 128, 256, 256, 3, 1, 1)],
    "wino": _s1([(8, 64, 512, 64, 64), (8, 64, 256, 128, 128), (4, 64, 128, 256, 256)]),
    "half": [(8, 64, 512, 64, 128, 3, 1, 1), (8, 64, 256, 128, 128, 3, 1, 1), (4, 64, 128, 256, 256, 3, 1, 1)],
    "pair": _s12([(8, 64, 512, 64, 128), (8, 64, 256, 128, 256)]),
}
_ONE_CHUNK = {"direct": (1, 1, 32, 64, 64, 3, 1, 1), "wino": (1, 2, 16, 128, 64, 3, 1, 1), "half": (1, 2, 64, 64, 128, 3, 1, 1),
              "pair": (1, 2, 32, 64, 64, 3, 1, 2)}
_MIXED = {
    # 3x3 and 1x1, strides (1,1), (1,2), (2,2): five kernel instantiations
    "direct": [(2, 16, 128, 64, 64, 3, 1, 1), (2, 8, 256, 64, 128, 3, 1, 2), (2, 16, 128, 128, 256, 3, 2, 2), (2, 8, 128, 64, 128, 1, 1, 2),
               (2, 8, 64, 128, 256, 1, 2, 2), (2, 8, 90, 128, 128, 3, 1, 1), (2, 8, 45, 64, 128, 3, 2, 2), (1, 5, 45, 64, 64, 1, 1, 2)],
    # 128-wide output blocks with 64- and 32-pixel chunks, 64-wide blocks, strided and 1x1 layers
    "half": [(2, 16, 128, 64, 128, 3, 1, 1), (2, 16, 128, 64, 64, 3, 1, 1), (2, 8, 32, 128, 128, 3, 1, 1), (2, 8, 256, 64, 128, 3, 1, 2),
             (2, 8, 64, 128, 256, 1, 2, 2), (2, 8, 180, 64, 64, 3, 1, 1), (1, 6, 90, 128, 128, 3, 1, 1), (2, 8, 45, 64, 128, 3, 2, 2)],
    # images that divide into chunks of 8 tiles and images that do not
    "wino": _s1([(2, 16, 128, 128, 128), (2, 8, 90, 128, 128), (2, 8, 64, 256, 256), (2, 5, 45, 128, 128), (2, 16, 128, 64, 64), (2, 8, 180, 64, 64)]),
    # (one instantiation whatever the table: the odd- and even-pixel items of three layers)
    "pair": _s12([(2, 8, 256, 64, 128), (2, 16, 128, 128, 256), (1, 8, 64, 64, 64)]),
}
_BAD_FIELD = {"direct": (2, 8, 64, 96, 128, 3, 1, 1), "wino": (2, 8, 64, 64, 128, 3, 1, 2), "half": (2, 8, 64, 64, 100, 3, 1, 1),
              "pair": (2, 7, 64, 64, 128, 3, 1, 2)}
# past the 32-bit offsets: refused by the half, Winograd and pixel-pair families; the direct family takes its kernel without the 32-bit fast path
_HUGE = {"direct": (1, 4096, 4096, 64, 64, 3, 1, 1), "wino": (1, 4096, 4096, 64, 64, 3, 1, 1), "half": (1, 4096, 4096, 64, 64, 3, 1, 1),
         "pair": (8, 64, 2 ** 16, 256, 256, 3, 1, 2)}


def tables():
    """[(name, family, dtype, n, layers)]: n is what the entry point is told, len(layers) lines follow."""
    out = []
    for fam, dtypes in DTYPES.items():
        for dt in dtypes:
            def add(name, layers, n=None):
                out.append((f"{fam}-{dt}-{name}", fam, dt, len(layers) if n is None else n, list(layers)))
            for (B, H, W) in ((8, 64, 2048), (1, 64, 720)):
                layers = trunk_layers(B, H, W)
                if fam == "half":
                    part = layers
                elif fam == "pair" and W == 720:
                    # (the pixel-pair family takes no layer of this image -- a width of 180 is no multiple of 32, ring_conv keeps its
                    # two stride-(1,2) layers direct: recorded as the refusal it is)
                    part = [l for l in layers if l[5:] == (3, 1, 2)]
                else:
                    part = trunk_family(layers, fam)
                add(f"trunk-{H}x{W}-b{B}", part)
            add("one-layer", _BIG[fam][:1])
            add("full-table", (_BIG[fam] * BATCH)[:BATCH])
            add("mixed-groups", _MIXED[fam])
            add("one-chunk-beside-large", [_BIG[fam][0], _ONE_CHUNK[fam]] + _BIG[fam][1:])
            add("digest", DIGEST[fam])
            add("refused-n-zero", [], 0)
            add("refused-n-above-table", (_BIG[fam] * (BATCH + 1))[:BATCH + 1])
            add("refused-field", [_BIG[fam][0], _BAD_FIELD[fam]])
            add("past-32-bit-offsets", [_BIG[fam][0], _HUGE[fam]])
    return out


def dump(tabs):
    """Run the program once over all tables; {name: {bytes, bytes_error, rc, error, plan}}."""
    text = "".join(f"{fam} {dt} {n}\n" + "".join(" ".join(str(v) for v in l) + "\n" for l in layers) for _, fam, dt, n, layers in tabs)
    env = {k: v for k, v in os.environ.items() if k != "DL_SWGRAD_ALL12"}
    res = subprocess.run([DUMP], input=text, capture_output=True, text=True, check=True, env=env)
    out, cur = {}, None
    for line in res.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "table":
            cur = {"bytes": None, "bytes_error": None, "rc": None, "error": None, "plan": []}
            out[tabs[int(rest.split()[0])][0]] = cur
        elif key in ("bytes", "rc"):
            cur[key] = int(rest)
        elif key in ("bytes_error", "error"):
            cur[key] = rest
        elif key == "plan":
            cur["plan"].append(rest)
    assert len(out) == len(tabs), res.stdout[-2000:]
    return out


@pytest.fixture(scope="module")
def dumped():
    return dump(tables())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _slabs(plan_line):
    return [int(w.split("=")[1]) for w in plan_line.split() if w.startswith("slabs=")]


def test_the_set_of_tables_is_the_recorded_one(golden):
    assert sorted(golden) == sorted(name for name, *_ in tables())


@pytest.mark.parametrize("name", [name for name, *_ in tables()])
def test_bytes_codes_messages_and_plan_text_are_the_recorded_ones(name, dumped, golden):
    got, exp = dumped[name], golden[name]
    for key in ("bytes", "bytes_error", "rc", "error"):
        assert got[key] == exp[key], (name, key, got[key], exp[key])
    assert got["plan"] == exp["plan"], "\n".join([name, "got:"] + got["plan"] + ["recorded:"] + exp["plan"])


def test_the_tables_reach_what_they_are_meant_to_reach(dumped):
    """Read from the plan text itself: several launch groups where a family has them, a table of one slab beside split layers, the
    full table, and the three refusals with the texts callers and tests read."""
    for fam, dtypes in DTYPES.items():
        for dt in dtypes:
            d = {k.split("-", 2)[2]: v for k, v in dumped.items() if k.startswith(f"{fam}-{dt}-")}
            first = {name: [l for l in v["plan"] if "reduce" not in l and "_sum_" not in l and "_out_" not in l] for name, v in d.items()}
            for name in ("one-chunk-beside-large", "digest"):
                slabs = [s for l in first[name] for s in _slabs(l)]
                assert d[name]["rc"] == 0 and 1 in slabs and max(slabs) > 1, (fam, dt, name, d[name])
            for name in ("mixed-groups", "digest"):
                assert len(first[name]) >= (1 if fam == "pair" else 2), (fam, dt, name, first[name])
            assert d["one-layer"]["rc"] == 0 and len(first["one-layer"]) == 1
            assert sum(len(_slabs(l)) for l in first["full-table"]) == BATCH * (2 if fam == "pair" else 1)
            for name in ("refused-n-zero", "refused-n-above-table"):
                assert d[name]["bytes"] == 0 and d[name]["rc"] == -1 and f"1..{BATCH} layers" in d[name]["error"] and not d[name]["plan"]
            bad = d["refused-field"]
            assert bad["bytes"] == 0 and bad["rc"] == -3 and "layer 1" in bad["error"] and bad["error"] == bad["bytes_error"] and not bad["plan"]
            huge = d["past-32-bit-offsets"]
            if fam == "direct":
                assert huge["rc"] == 0 and "true>" not in first["past-32-bit-offsets"][0]
            else:
                assert huge["bytes"] == 0 and huge["rc"] == -3 and "layer 1" in huge["error"]
            assert d["trunk-64x2048-b8"]["rc"] == 0 and d["trunk-64x2048-b8"]["bytes"] > 0


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_wgrad_batch_plan_host --record")
    with open(GOLDEN, "w") as f:
        json.dump(dump(tables()), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", GOLDEN)
