#!/usr/bin/env python3
"""Instruction mix of the direct fp32 convolution kernels in a hipcc -S listing of csrc/conv.hip (the method of isa_hist.py, one line
per instantiation): the chunk loop (the outermost loop with MFMAs) as MFMA / VALU / SALU / VMEM, the VALU before and after it, and the
trailer's Occupancy / LDS bytes / ScratchSize.

    isa_table.py conv.s [--lib libdelora_hip.so] [substring of the demangled name ...]

Without substrings the rows are what the dispatch itself selects (dl_conv_plan_describe at 256 CUs, of the library given by --lib,
default the built one) for the strided 3x3 and the 1x1 layers of the benchmark's network -- forward, input gradient, merged weight
gradient -- so the table cannot drift away from the dispatch; every 1x1 k_conv_f32 row is also listed at the other chunk depths the
listing holds, to set a choice of depth against its alternative."""
import os
import re
import subprocess
import sys

# (H, W, C, K, stride) of the three down-sampling blocks at batch 8, 64 x 2048 scans (bench.py)
BLOCKS = [(64, 512, 64, 128, (1, 2)), (64, 256, 128, 256, (1, 2)), (64, 128, 256, 512, (2, 2))]


def plan_rows(lib_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from delora_amd import _lib as L
    if lib_path: L.LIB_PATH = lib_path
    rows = []
    for H, W, C, K, st in BLOCKS:
        for ks in (3, 1):
            for op, mode in ((L.PLAN_CONV, 0), (L.PLAN_DGRAD_STRIDED, int(ks == 1)), (L.PLAN_WGRAD_BATCH, 0)):
                for line in L.conv_plan(op, 0, 8, H, W, C, K, ks, st[0], st[1], mode, 256):
                    name = line.split(" grid=")[0]
                    if name and not name.startswith("k_wgrad_reduce") and name not in rows: rows.append(name)
    return rows


def kind(op):
    if op.startswith("v_mfma"): return "MFMA"
    if op.startswith("v_"): return "VALU"
    if op.startswith("s_"): return "SALU"
    if op.startswith(("global", "buffer", "flat")): return "VMEM"
    if op.startswith("ds_"): return "LDS"
    return None


def main():
    args = sys.argv[1:]
    lib_path = args.pop(args.index("--lib") + 1) if "--lib" in args else None
    if "--lib" in args: args.remove("--lib")
    txt = open(args[0]).read().split("\n")
    subs = args[1:]
    want = subs or plan_rows(lib_path)
    if not subs:      # the 1x1 rows at the other chunk depths
        want += [v for w in list(want) for ck in (16, 32) for v in [re.sub(r"^(k_conv_f32<128, 64, )\d+(, \d+, Geom\w+<1, )", rf"\g<1>{ck}\2", w)] if v not in want]
    starts = [(i, m.group(1)) for i, l in enumerate(txt) for m in [re.match(r"^(_Z\w+):", l)] if m]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in starts), capture_output=True, text=True).stdout.split("\n")
    print("instantiation | loop MFMA / VALU / SALU / VMEM | VALU/MFMA | VALU before | VALU after | Occupancy | LDS bytes | ScratchSize")
    for (a, _), dem in zip(starts, names):
        dem = dem.replace("void ", "").split("(")[0]
        if not any(w == dem for w in want) and not (subs and any(w in dem for w in want)): continue
        b = next(i for i in range(a, len(txt)) if txt[i].startswith(".Lfunc_end"))
        lines = txt[a:b + 1]
        labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
        ops = [(l.split() or [""])[0] for l in (x.strip() for x in lines)]
        kinds = [None if (not o or o[0] in ";.") else kind(o) for o in ops]
        best = None
        for i, l in enumerate(lines):
            m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)
            if m and labels.get(m.group(1), 1 << 30) < i:
                x = labels[m.group(1)]
                n = kinds[x:i + 1].count("MFMA")
                if n and (best is None or i - x > best[1] - best[0]): best = (x, i)
        x, y = best
        c = {k: kinds[x:y + 1].count(k) for k in ("MFMA", "VALU", "SALU", "VMEM")}
        tail = "\n".join(txt[b:b + 200])
        occ = re.search(r"; Occupancy: (\d+)", tail).group(1)
        scr = re.search(r"; ScratchSize: (\d+)", tail).group(1)
        lds = re.search(r"; LDSByteSize: (\d+)", tail).group(1)
        print(f"{dem} | {c['MFMA']} / {c['VALU']} / {c['SALU']} / {c['VMEM']} | {c['VALU'] / c['MFMA']:.2f} | {kinds[:x].count('VALU')} | "
              f"{kinds[y + 1:].count('VALU')} | {occ} | {lds} | {scr}")


if __name__ == "__main__":
    main()
