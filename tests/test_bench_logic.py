"""Host-side logic of bench.py and of the PMC tooling it drives (no GPU): the roofline object built from launch-profile rows, and the
mapping of rocprofv3 counter dispatches back to profile rows."""
import csv
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_roofline_object_from_profile_rows():
    """conv_roofline: dominant family by summed time, algorithmic flop / kernel time against the dense peak of its arithmetic type, per-shape
    rows, launches per step taken over the steps that actually carried events."""
    import bench
    args = bench.parse(["--steps", "20"])
    rows = [  # 5 evented steps: 6 launches of a 256-channel shape per step, 8 of a 64-channel shape, one direct launch
        {"name": "k_wino_conv conv N8 64x128 C256 K256 3x3 s(1,1)", "launches": 30, "ms": 30 * 0.335, "flop": 30 * 34.36e9, "bytes": 30 * 138e6},
        {"name": "k_wino_conv conv N8 64x512 C64 K64 3x3 s(1,1)", "launches": 40, "ms": 40 * 0.107, "flop": 40 * 8.59e9, "bytes": 40 * 134e6},
        {"name": "k_conv_f32 fwd N8 64x512 C64 K128 3x3 s(1,2)", "launches": 5, "ms": 5 * 0.23, "flop": 5 * 19.3e9, "bytes": 5 * 100e6},
    ]
    bench.LIVE_PMC["rows"] = {rows[0]["name"]: 312_000_000, rows[1]["name"]: 193_000_000}
    try:
        roof, prof = bench.conv_roofline(rows, args, step_ms=14.6, prof_steps=5)
    finally:
        bench.LIVE_PMC["rows"] = None
    assert roof["kernel"].startswith("k_wino_conv") and roof["bound"] == "mfma" and roof["peak"] == bench.MFMA_F32_PEAK_TFLOPS
    tf = (30 * 34.36e9 + 40 * 8.59e9) / (30 * 0.335 + 40 * 0.107) * 1e-9
    assert roof["achieved"] == pytest.approx(tf, rel=1e-3) and roof["frac"] == pytest.approx(tf / 157.3, abs=2e-4)
    assert roof["launches_per_step"] == 14.0 and roof["ms_per_step"] == pytest.approx((30 * 0.335 + 40 * 0.107) / 5, rel=1e-3)
    by = {l["launch"]: l for l in roof["layers"]}
    assert by[rows[0]["name"]]["launches_per_step"] == 6.0 and by[rows[0]["name"]]["traffic_MB_per_launch"] == 312.0
    assert by[rows[1]["name"]]["frac"] == pytest.approx(8.59e9 / 0.107e-3 * 1e-12 / 157.3, abs=2e-4)
    assert roof["traffic"] == int(1e6 * (312.0 * 6 + 193.0 * 8) / 14)          # launch-weighted mean of the layer rows
    assert prof["families_ms_per_step"]["k_conv_f32"] == pytest.approx(0.23, rel=1e-3)


def test_counter_dispatches_map_back_to_profile_rows(tmp_path):
    """tools/conv_layers_pmc.traffic_rows: every op runs twice (warm-up + measured) -- the measured dispatches of a family are taken in
    order; the same kernel on the same shape in two passes (Winograd forward / input gradient) is a launch-weighted mean; gfx950 x2 on reads."""
    m = _load(os.path.join(ROOT, "tools", "conv_layers_pmc.py"), "conv_layers_pmc")

    def table(path, counter, seq):
        with open(path, "w") as f:
            w = csv.DictWriter(f, fieldnames=["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"])
            w.writeheader()
            for i, (k, v) in enumerate(seq):
                w.writerow({"Dispatch_Id": i, "Kernel_Name": k, "Counter_Name": counter, "Counter_Value": v})
    wino, conv = "void k_wino_conv<32>(WinoArgs)", "void k_conv_f32<128, 64, 8, 128, GeomConv<3, 1, 2>, false, 2>(ConvArgs)"
    seq = [(wino, 1), (wino, 100), ("at::native::fill", 7), (wino, 2), (wino, 200), (conv, 3), (conv, 4), (conv, 30), (conv, 40)]
    table(tmp_path / "f.csv", "FETCH_SIZE", seq)
    table(tmp_path / "w.csv", "WRITE_SIZE", [(k, v / 2) for k, v in seq])
    order = {"workload": "x", "order": [
        {"op": "fwd", "row": "k_wino_conv conv A", "launches": 1, "compulsory_bytes": 10},
        {"op": "dgrad", "row": "k_wino_conv conv A", "launches": 1, "compulsory_bytes": 10},
        {"op": "phases", "row": "k_conv_f32 dgrad B", "launches": 2, "compulsory_bytes": 5}]}
    rows = m.traffic_rows(order, str(tmp_path / "f.csv"), str(tmp_path / "w.csv"))
    a = rows["k_wino_conv conv A"]
    assert a["kernel_launches"] == 2 and a["read_bytes_corrected_x2"] == (100 + 200) * 1024 * 2 and a["write_bytes"] == (50 + 100) * 1024
    assert a["hbm_bytes_per_launch"] == ((100 + 200) * 2048 + 150 * 1024) // 2
    b = rows["k_conv_f32 dgrad B"]
    assert b["kernel_launches"] == 2 and b["read_bytes_corrected_x2"] == (30 + 40) * 2048 and b["hbm_bytes_per_launch"] == ((30 + 40) * 2048 + 35 * 1024) // 2


def test_epilogue_tanh_formula_in_float32_emulation():
    """The constants of csrc/common.h: dl_tanh, read from the source and evaluated with float32 roundings in numpy: odd polynomial below
    the switch point, 1 - 2 / (2^(2 log2(e) |x|) + 1) above -- both within 2 ulp of float64 tanh (the GPU test measures 1.4 ulp
    including the hardware's exp2 / rcp)."""
    import re
    import numpy as np
    src = open(os.path.join(ROOT, "delora_amd", "csrc", "common.h")).read()
    body = src[src.index("float dl_tanh(float x)"):]
    body = body[:body.index("}")]
    coef = [np.float32(v) for v in re.findall(r"(-?\d+\.\d+(?:e-?\d+)?)f", body)]
    # order in the source: p = c4; fma c3, c2, c1, c0; exp2 scale; the constants 1.f / -2.f / 1.f; the switch point
    c4, c3, c2, c1, c0 = coef[:5]
    scale = np.float32(2.885390081777927)
    assert scale in coef and np.float32(0.625) in coef
    f32 = np.float32
    x = np.concatenate([np.linspace(0, 0.625, 100001)[:-1], np.linspace(0.625, 12.0, 200001), np.logspace(-30, -3, 2000)]).astype(f32)
    t = (x * x).astype(f32)
    p = np.full_like(x, c4)
    for c in (c3, c2, c1, c0):
        p = (p.astype(np.float64) * t + np.float64(c)).astype(f32)                         # fmaf: one rounding
    lo = ((x * t).astype(f32).astype(np.float64) * p + x.astype(np.float64)).astype(f32)
    e = np.exp2((x * scale).astype(f32).astype(np.float64)).astype(f32)
    q = (1.0 / (e.astype(np.float64) + 1.0).astype(f32).astype(np.float64)).astype(f32)
    hi = (q.astype(np.float64) * -2.0 + 1.0).astype(f32)
    got = np.where(x < f32(0.625), lo, hi).astype(np.float64)
    ref = np.tanh(x.astype(np.float64))
    ulp = np.spacing(np.maximum(np.abs(ref), 1e-45).astype(f32)).astype(np.float64)
    err = np.abs(got - ref) / ulp
    assert err.max() < 2.0, (float(err.max()), float(x[err.argmax()]))


def test_half_epilogue_tanh_formula_in_float32_emulation():
    """csrc/convh_common.h: ch_tanh / ch_tanh2 (the bf16 / fp16 kernels' epilogue), constants read from the source: x P(x^2) / Q(x^2) on
    the argument clamped to [-6, 6], evaluated with float32 roundings (fused multiply-adds, a correctly rounded reciprocal): relative
    error below 5 % of an fp16 rounding (2^-11) over the whole axis, odd, monotone where the storage type can see it."""
    import re
    import numpy as np
    src = open(os.path.join(ROOT, "delora_amd", "csrc", "convh_common.h")).read()
    c = {k: np.float32(v) for k, v in re.findall(r"#define CH_TANH_(\w+) (-?[\d.]+(?:e-?\d+)?)f", src)}
    assert set(c) == {"CLAMP", "P0", "P1", "P2", "Q1", "Q2", "Q3"}, sorted(c)
    f32 = np.float32

    def fma(a, b, d):
        return (a.astype(np.float64) * b.astype(np.float64) + np.float64(d)).astype(f32)

    x = np.concatenate([np.linspace(-12, 12, 400001), np.logspace(-38, 0, 20001), -np.logspace(-38, 0, 20001)]).astype(f32)
    xc = np.clip(x, -c["CLAMP"], c["CLAMP"])
    u = (xc * xc).astype(f32)
    p = fma(fma(np.full_like(u, c["P2"]), u, c["P1"]), u, c["P0"])
    q = fma(fma(fma(np.full_like(u, c["Q3"]), u, c["Q2"]), u, c["Q1"]), u, f32(1))
    got = ((xc * p).astype(f32) * (f32(1) / q).astype(f32)).astype(f32).astype(np.float64)
    ref = np.tanh(x.astype(np.float64))
    m = ref != 0
    rel = np.abs(got[m] - ref[m]) / np.abs(ref[m])
    assert rel.max() < 0.05 * 2.0 ** -11, (float(rel.max()), float(x[m][rel.argmax()]))
    assert np.array_equal(got, -got[::-1]) or np.allclose(got[:400001], -got[:400001][::-1], rtol=0, atol=0)      # odd
    assert np.all(np.abs(got) < 1.0)


def test_launch_plan_never_lets_a_single_process_pose_as_n_ranks():
    """`python bench.py --gpus 8` started as ONE plain process must become 8 ranks (re-launch under torch.distributed.run) or stop --
    never run one rank and print it as an 8-GPU number (bench.py:563 used to fall through)."""
    import bench
    argv = ["/x/bench.py", "--gpus", "8", "--steps", "3"]
    # a plain process, 8 GPUs visible: re-launch with one rank per GPU, rendezvous on 127.0.0.1
    action, cmd = bench.launch_plan(8, {}, 8, argv, free_port=lambda: 40123)
    assert action == "spawn"
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "40123" and cmd[-len(argv):] == argv
    # a rank of a correctly sized job, and the single-GPU default: just run
    assert bench.launch_plan(8, {"WORLD_SIZE": "8", "RANK": "3"}, 8, argv) == ("run", None)
    assert bench.launch_plan(1, {}, 1, argv) == ("run", None)
    assert bench.launch_plan(1, {}, 8, argv) == ("run", None)
    # WORLD_SIZE disagrees with --gpus (either direction), too few GPUs for the ranks: refuse
    for env, gpus, seen in (({"WORLD_SIZE": "2", "RANK": "0"}, 8, 8), ({"WORLD_SIZE": "8", "RANK": "0"}, 1, 8), ({}, 8, 1),
                            ({"WORLD_SIZE": "8", "RANK": "0"}, 8, 4), ({}, 0, 1)):
        with pytest.raises(SystemExit):
            bench.launch_plan(gpus, env, seen, argv)
    # the share-GPU test hook is the only way to put several ranks on one device
    action, cmd = bench.launch_plan(2, {"DELORA_BENCH_SHARE_GPU": "1", "MASTER_PORT": "29533"}, 1, argv)
    assert action == "spawn" and cmd[cmd.index("--master-port") + 1] == "29533"
    assert bench.launch_plan(2, {"DELORA_BENCH_SHARE_GPU": "1", "WORLD_SIZE": "2", "RANK": "1"}, 1, argv) == ("run", None)


def test_weight_gradient_takes_the_parameters_strides():
    """DistributedDataParallel (gradient_as_bucket_view) compares the strides of a gradient with those of its parameter literally: the
    1x1 down-sampling weights [512,256,1,1] keep strides (256,1,1,1) in channels_last storage while the permuted kernel output
    [K,1,1,C] has (256,1,256,256) -- one extra copy per bucket and step (GPUTEST r03 warning)."""
    import torch
    from delora_amd.models.ring_conv import grad_for
    for make in (lambda: torch.empty(512, 256, 1, 1).contiguous(memory_format=torch.channels_last),
                 lambda: torch.empty(512, 256, 1, 1).to(memory_format=torch.channels_last),
                 lambda: torch.empty(128, 64, 3, 3).contiguous(memory_format=torch.channels_last)):
        w = make()
        K, C, ks = w.shape[0], w.shape[1], w.shape[2]
        dw = torch.randn(K, ks, ks, C)
        for ref in (w, (tuple(w.shape), tuple(w.stride()))):
            g = grad_for(dw, ref)
            assert g.shape == w.shape and g.stride() == w.stride() and g.data_ptr() == dw.data_ptr()
            assert torch.equal(g, dw.permute(0, 3, 1, 2))


def test_kernel_sum_of_trace_cuts_steps_at_the_projection():
    """bench.kernel_sum_of_trace: a kernel trace is cut into steps at `k_project_scatter`; the median step's summed kernel time and
    start-to-start time are what `shipped_config.batch_1.kernel_sum` reports."""
    import bench
    rows, t = [], 1000
    for step in range(6):
        for name, dur, gap in (("k_fill_words", 2000, 500), ("k_project_scatter(float const*)", 10000, 500), ("k_other", 30000 + 1000 * (step == 2), 1500)):
            if name == "k_fill_words":
                pass
            rows.append({"Kernel_Name": name, "Start_Timestamp": str(t), "End_Timestamp": str(t + dur)})
            t += dur + gap
    out = bench.kernel_sum_of_trace(rows, steps=5)
    assert out["kernels_per_step"] == 3 and out["steps_in_trace"] == 4
    assert abs(out["kernel_sum_ms"] - 42000e-6) < 1e-9 and abs(out["step_wall_ms"] - 44500e-6) < 1e-9
    assert bench.kernel_sum_of_trace(rows[:5], steps=5) is None


def test_convergence_seeds_study_intervals_overlap():
    """profiles/r06_convergence_seeds.json (tools/convergence_seeds.py on an MI355X: 5 training seeds x {float32, bfloat16} x {trunk as one
    autograd Function, cut per layer as a DDP rank runs it}, scenes with cross-walls and pillars): the claim DESIGN.md section 8 makes is
    statistical -- the precisions and the cuts end within each other's spread -- and this test holds the committed numbers to it: every
    cell has >= 5 runs, the means of every pair of cells differ by less than the sum of their standard deviations (final loss: plus 5 %
    of the value, the bf16 runs' spread being tiny), every run beats the "mean motion" yardstick's rotation error and the "no motion"
    translation error by a factor of five and ends below 0.9 of its first epochs' loss (one float32 run of the ten sits on a higher
    plateau, 0.55 against 0.43: that is what the float32 cells' standard deviation is)."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = json.load(open(os.path.join(root, "profiles", "r06_convergence_seeds.json")))
    cells = d["cells"]
    assert set(cells) == {"float32/mono", "bfloat16/mono", "float32/layer", "bfloat16/layer"}
    assert all(c["n"] >= 5 for c in cells.values()) and d["hip_graph"] is False
    names = sorted(cells)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for key, slack in (("final_loss", 0.05), ("t_rel_percent", 0.0), ("r_rel_deg_per_m", 0.0)):
                ma, mb = cells[a][key]["mean"], cells[b][key]["mean"]
                assert abs(ma - mb) <= cells[a][key]["sd"] + cells[b][key]["sd"] + slack * max(ma, mb), (a, b, key, ma, mb)
    for r in d["runs"]:
        assert r["t_rel_percent"] < r["yardstick_no_motion_percent"] / 5.0 and r["final_loss"] < 0.9 * r["first_loss"], r


def test_plain_run_is_the_default_and_full_is_opt_in():
    """A plain `bench.py` run measures the headline only; `--full` asks for every other leg; `--dump-outputs` names a directory."""
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs == "" and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_are_float_files_under_the_size_limit(tmp_path):
    """write_outputs: DIR/<name>.npy, float32 kept, everything else float64; more than 64 MB in all is refused.  The weight / gradient
    sample is a fixed, sorted set of distinct indices (the same in every run), all indices when there are fewer than the sample size."""
    import numpy as np
    import bench
    names = bench.write_outputs(str(tmp_path / "d"), {"a": np.ones((2, 4, 4), np.float32), "b": np.arange(3), "c": 1.5})
    assert names == ["a", "b", "c"]
    a, b, c = (np.load(tmp_path / "d" / f"{n}.npy") for n in names)
    assert a.dtype == np.float32 and a.shape == (2, 4, 4) and b.dtype == np.float64 and b.tolist() == [0.0, 1.0, 2.0] and c.dtype == np.float64
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "e"), {"x": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "e").exists()
    i1, i2 = bench.dump_sample_indices(12_000_000), bench.dump_sample_indices(12_000_000)
    assert np.array_equal(i1, i2) and len(i1) == bench.DUMP_SAMPLE and np.all(np.diff(i1) > 0) and 0 <= i1[0] and i1[-1] < 12_000_000
    assert np.array_equal(bench.dump_sample_indices(10), np.arange(10))
