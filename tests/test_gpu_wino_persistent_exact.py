"""The persistent loop of k_wino_conv (csrc/wino_conv_body.h) BIT FOR BIT against the float64 reference and the direct kernel, on
small-integer data in poisoned arenas (the method of tests/test_gpu_conv_exact.py), at launches with MORE TILE GROUPS THAN CUs.

The grid of a launch without a split is capped at the CU count and a workgroup walks the groups grp, grp + grid, ...  Between two
groups it requests raw(0), raw(1) and U(0) of the next group by LDS DMA while the epilogue of the group in hand runs in the lower
(V, U) buffer, waits for them, transforms V(0) of the next group and only then stores its own results; the accumulators are never
zeroed, and the output offsets are taken before the group variables move on.  Every other exact test launches at most 96 groups, so
that code never ran under them.  The cases (``conv_exact_cases.persistent_cases``) are sized by the CU count of the device:
cu < groups < 2 cu for each of the six non-split instantiations (a workgroup's second group lies in another image), one geometry
whose second group lies in the same image, two with at least 3 cu groups (a middle group, which follows one and prefetches one),
one with 72 input channels (nine chunks: the last chunk of a group sits in the buffer the next group's U(0) arrives in) and one with
several output blocks whose number does not divide a workgroup's step, so that k0 changes across a hand-over.  Before any
launch each test asserts from the device's own dispatch that the grid is smaller than the number of groups.

Forward and input gradient only: the weight gradients are not persistent kernels (and a batch of this size leaves their sums no
headroom).  Every tail of the stride-1 exact test, plus forward tanh against the direct kernel (the same ``dl_tanh`` on the same
value: equal to the bit although neither equals float64) -- tanh and the plain tails take ``wn_store_items``, relu the generic store
loop.  Every call runs twice and must repeat itself.
"""
import pytest
import torch

from tests import conv_exact_cases as cc
from tests import conv_ref as cr
from tests import util
from tests.test_gpu_conv_exact import ACT, BWD_TAILS, FWD_TAILS, TANH, Run, _conv_call, _dev, _guarded, _prepared_weights, _wino_call, wino_plan_line

pytestmark = pytest.mark.gpu

NAMES = list(cc.persistent_cases(256))                # (the names do not depend on the CU count)


def where_in_the_walk(got, ref, case, transposed, what):
    """Printed for a mismatch: the tile groups that hold wrong elements, and whether each of them follows another group of its
    workgroup (the hand-over) or is a workgroup's first (the prologue)."""
    grid, tr, tc, table = cc.group_table(case, 0, transposed)
    bad = torch.nonzero(got.detach().cpu() != ref.to(got.dtype))
    if not len(bad):
        return
    hit = {(int(n), int(h) // (2 * tr), int(w) // (2 * tc), int(k) // 64) for n, h, w, k in bad.tolist()}
    first, later = set(table[:grid]), set(table[grid:])
    print(f"{what}: wrong elements in {len(hit)} tile groups (image, group row, group column, channel block): {sorted(hit)[:12]}")
    print(f"    {len(hit & later)} of them follow another group of their workgroup, {len(hit & first)} are a workgroup's first group; "
          f"{len(later)} groups follow another one in this launch")
    if hit <= later:
        print("    ALL mismatches lie in groups that follow another group of their workgroup")


def _twice(r, call, out, what):
    """The same call again into the same buffer: a persistent workgroup must not depend on what its LDS or registers held."""
    first = out.clone()
    call()
    torch.cuda.synchronize()
    r.A.check(f"{r.c.id} {what}, second run")                       # (guards and inputs after the repeated launch too)
    r.A.check_output(out, f"{r.c.id} {what}, second run")
    assert torch.equal(first, out), f"{r.c.id}: two runs of the same call differ ({what})"


def run_persistent(name, dev):
    cu = torch.cuda.get_device_properties(dev).multi_processor_count
    c = cc.persistent_cases(cu)[name]
    # ---- before any launch: the dispatch of this device walks several groups per workgroup, on the instantiation the name says
    for transposed in ((False, True) if c.dgrad_ok else (False,)):
        line = wino_plan_line(c, transposed)
        groups, grid = cc.wino_groups(line, c.N, c.H, c.W, c.C if transposed else c.K)
        _, _, same, other = cc.group_walk(c, 0, transposed)
        blocks = cc.block_changes(groups, grid, (c.C if transposed else c.K) // 64)[1]
        print(f"[persistent] {name} ({c.id}) {'input gradient' if transposed else 'forward'}: groups {groups}, grid {grid}, {cu} CUs; "
              f"hand-overs inside an image {same}, to another image {other}, to another channel block {blocks}")
        assert blocks > 0 or not name.endswith("several blocks"), f"{name}: k0 never changes between a workgroup's groups"
        tc, rag = name.split(" ")[0].strip("<>").split(",")
        assert line.startswith(f"k_wino_conv<{tc}, {'true' if rag == 'T' else 'false'}, false> grid="), line
        assert grid < groups, f"{name}: grid {grid} is not smaller than {groups} groups -- the launch is not persistent"
    r = Run(c, dev)
    wf, wb, uf, ub = _prepared_weights(r)
    yshape, xshape = tuple(r.y0.shape), tuple(r.x.shape)
    # ---- forward
    for i, (flags, act, kind) in enumerate(FWD_TAILS + [(ACT, TANH, None)]):
        add, sv, add_d, sv_d = r.tail_operands(yshape, flags, kind, 10 + 2 * i)
        y_dir, y_new = r.out(yshape, name="y (direct)"), r.out(yshape, name="y (Winograd)")

        def direct():
            _conv_call(r, r.x_d, wf, y_dir, add_d, sv_d, c.C, c.K, 3, (1, 1), 0, act, flags)

        def wino():
            _wino_call(r, r.x_d, uf, y_new, add_d, sv_d, c.C, c.K, act, flags)

        direct()
        wino()
        what = f"forward, tail {flags}/{act}"
        if act == TANH:                                   # not exact against float64; the two kernels must still agree to the bit
            torch.cuda.synchronize()
            r.A.check(f"{c.id} {what}")
            r.A.check_output(y_new, f"{c.id} {what}")
            r.A.check_output(y_dir, f"{c.id} {what}")
        else:
            ref = cr.epilogue(r.y0, flags, act, add, sv)
            r.compare(y_dir, ref, "direct " + what, (8, 64))
            if r.compare(y_new, ref, "Winograd " + what):
                where_in_the_walk(y_new, ref.float(), c, False, f"{c.id} Winograd {what}")
        n = cr.mismatches(y_new, y_dir.detach().cpu(), f"{c.id} Winograd against direct, {what}")
        if n:
            where_in_the_walk(y_new, y_dir.detach().cpu(), c, False, f"{c.id} Winograd against direct, {what}")
        r.bad += n
        _twice(r, direct, y_dir, "direct " + what)
        _twice(r, wino, y_new, "Winograd " + what)
    # ---- input gradient
    for i, (flags, act, kind) in enumerate(BWD_TAILS if c.dgrad_ok else []):
        add, sv, add_d, sv_d = r.tail_operands(xshape, flags, kind, 30 + 2 * i)
        ref = cr.epilogue(r.dx0, flags, act, add, sv)
        dx_dir, dx_new = r.out(xshape, name="dx (direct)"), r.out(xshape, name="dx (Winograd)")

        def direct():
            _conv_call(r, r.g_d, wb, dx_dir, add_d, sv_d, c.K, c.C, 3, (1, 1), 1, act, flags)

        def wino():
            _wino_call(r, r.g_d, ub, dx_new, add_d, sv_d, c.K, c.C, act, flags)

        direct()
        wino()
        what = f"input gradient, tail {flags}/{act}"
        r.compare(dx_dir, ref, "direct " + what, (8, 64))
        if r.compare(dx_new, ref, "Winograd " + what):
            where_in_the_walk(dx_new, ref.float(), c, True, f"{c.id} Winograd {what}")
        assert torch.equal(dx_dir, dx_new) or r.bad, f"{c.id}: Winograd and direct input gradient differ from each other ({what})"
        _twice(r, direct, dx_dir, "direct " + what)
        _twice(r, wino, dx_new, "Winograd " + what)
    return r.bad


@pytest.mark.parametrize("name", NAMES, ids=[n.translate(str.maketrans(" ", "-", "<>,")) for n in NAMES])
def test_several_groups_per_workgroup_equal_float64_and_the_direct_kernel(name):
    dev = _dev()
    bad = _guarded(run_persistent, name, dev)
    util.measured(f"persistent Winograd exact {name}: elements that differ", bad, bound=0)
