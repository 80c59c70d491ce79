"""tests/segpool_ref.py on the CPU: pool_ref against autograd through oracle/segpool_oracle.py, the span situations the fan-in
layouts are meant to contain, and the condition of every case of tests/test_hip_segpool_edges.py -- the float32 CPU oracle must
stay below a quarter of the bound the GPU test applies, and pool_ref with split-bf16 operands below half of it, so that what the
GPU test measures is the kernel and not the case."""
import numpy as np
import pytest
import torch

from oracle import segpool_oracle as orc
from tests import segpool_ref as sr
from tests.test_hip_segpool import OUT_TOL, grad_bound


def _autograd(c, dtype):
    to = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
    ox, ow, ob, oq = to(c.x), to(c.w), to(c.b), to(c.qv)
    out = orc.segment_pool(ox, ow, ob, oq, c.ptr.tolist(), c.idx.tolist())
    (out * torch.from_numpy(c.dout).to(dtype)).sum().backward()
    return sr.Ref(out.detach(), None, ox.grad, ow.grad, ob.grad, oq.grad)


def _small(kind):
    if kind == "partition":
        ptr, idx = sr.lengths_layout([5, 1, 12, 7], True, 1, 30)
    elif kind == "shared_rows":
        ptr, idx = sr.lengths_layout([5, 1, 12, 7, 40], False, 2, 11)
    elif kind == "empty_segment":
        ptr, idx = sr.lengths_layout([3, 0, 6, 0], False, 3, 9)
    else:
        ptr, idx = sr.lengths_layout([300, 2], False, 4, 50)
    return sr._make(kind, {"partition": 30, "shared_rows": 11, "empty_segment": 9, "long_segment": 50}[kind], 20, 8, kind == "partition",
                    ptr, idx, 17)


@pytest.mark.parametrize("kind", ["partition", "shared_rows", "empty_segment", "long_segment"])
def test_pool_ref_is_the_oracle_in_float64(kind):
    c = _small(kind)
    want = _autograd(c, torch.float64)
    got = sr.pool_ref(c.x, c.w, c.b, c.qv, c.ptr, c.idx, c.dout)
    for f in ("out", "dx", "dw", "db", "dq"):
        w = getattr(want, f).numpy()
        assert np.abs(getattr(got, f) - w).max() <= 1e-12 * np.abs(w).max(), (kind, f)
    sums = np.bincount(np.repeat(np.arange(len(c.ptr) - 1), np.diff(c.ptr)), got.alpha, len(c.ptr) - 1)
    assert np.allclose(sums[np.diff(c.ptr) > 0], 1.0, rtol=0, atol=1e-14) and (sums[np.diff(c.ptr) == 0] == 0).all()


def test_bf16_rounding_is_round_to_nearest_even():
    a = np.asarray([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -8 + 2.0 ** -20), 0.0])
    want = np.asarray([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 0.0])
    assert np.array_equal(sr.bf16_round(a), want)
    r = np.random.default_rng(0).standard_normal(4096) * 10.0 ** np.random.default_rng(1).integers(-6, 6, 4096)
    assert np.array_equal(sr.bf16_round(r), torch.from_numpy(r).float().bfloat16().double().numpy())


def test_layout_builders():
    ptr, idx = sr.lengths_layout(sr.LENGTHS, True, 5, sum(sr.LENGTHS) + 9)
    assert np.diff(ptr).tolist() == list(sr.LENGTHS) and len(set(idx.tolist())) == len(idx) == sum(sr.LENGTHS)
    ptr, idx = sr.lengths_layout(sr.LENGTHS, False, 5, 300)
    assert np.diff(ptr).tolist() == list(sr.LENGTHS) and idx.min() >= 0 and idx.max() < 300 and len(set(idx.tolist())) < len(idx)
    for mult in sr.FANIN.values():
        ptr, idx = sr.fanin_layout(mult, 3)
        assert np.bincount(idx, minlength=len(mult)).tolist() == list(mult)
        assert ptr[0] == 0 and ptr[-1] == sum(mult) and np.diff(ptr).min() >= 1 and np.diff(ptr).max() <= 90
        order = np.argsort(idx, kind="stable")                              # what the backward's sort leaves: row r's run
        p = np.concatenate([[0], np.cumsum(mult)])
        for r in range(len(mult)):
            assert (idx[order[p[r]:p[r + 1]]] == r).all()
        assert any(len(set(idx[a:b].tolist())) < b - a for a, b in zip(ptr[:-1], ptr[1:]))          # a repeat inside a segment


def test_fanin_layouts_sit_where_the_span_path_branches():
    """Every situation of seg_span_gather_kernel / seg_row_combine_kernel occurs in a named layout, and the runs are the ones the
    cases' comments state."""
    a, b = sr.span_classes(sr.FANIN["fan_a"]), sr.span_classes(sr.FANIN["fan_b"])
    assert set().union(*a) == set(sr.SPAN_CLASSES)
    assert set().union(*b) == set(sr.SPAN_CLASSES) - {"padded_tail"} and sum(sr.FANIN["fan_b"]) == 768
    assert sum(sr.FANIN["fan_a"]) == 779 and -(-779 // 64) * 64 == 832
    assert a == [{"owned", "ends_on_boundary"}, {"owned"}, {"owned", "ends_on_boundary"}, {"slot0"}, {"owned", "ends_on_boundary"},
                 {"slot0", "ends_on_boundary"}, set(), {"slot0", "inner"}, {"owned"}, {"slot1", "inner"}, {"slot1"}, {"owned", "padded_tail"}]
    assert b == [{"owned"}, {"owned", "ends_on_boundary"}, {"owned", "ends_on_boundary"}, {"slot0", "inner"}, {"owned", "ends_on_boundary"}, set(),
                 {"slot0", "inner", "ends_on_boundary"}, {"owned", "ends_on_boundary"}, {"owned"}, {"slot1", "ends_on_boundary"},
                 {"owned", "ends_on_boundary"}]
    # the other shared-rows cases: which situations their (random) lists happen to reach is stated, not assumed
    for name in ("len_shared_20", "padded_lists"):
        c = sr.case(name)
        got = set().union(*sr.span_classes(np.bincount(c.idx, minlength=c.R)))
        assert {"owned", "slot1"} <= got, (name, got)


def test_cases_are_what_they_claim():
    for name in sr.case_names():
        c = sr.case(name)
        n = np.bincount(c.idx, minlength=c.R)
        assert c.ptr[0] == 0 and (np.diff(c.ptr) >= 0).all() and c.ptr[-1] == len(c.idx) and (c.idx >= 0).all() and (c.idx < c.R).all()
        assert (n.max() <= 1) if c.partition else (n.max() > 1), name
    assert sorted(np.diff(sr.case("len_part_20").ptr)) == [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 257, 1000]
    assert (np.bincount(sr.case("len_part_300").idx, minlength=sr.case("len_part_300").R) == 0).sum() == 9
    assert (np.bincount(sr.case("rows_orphans").idx, minlength=129) == 0).sum() == 9
    for R in sr.ROW_COUNTS:
        assert len(sr.case("rows_%d_128" % R).idx) == 128 and len(sr.case("rows_%d_100" % R).idx) == 100
    lists = sr.padded_lists()
    assert (lists == -1).any(1).all() and (lists[5] == -1).all() and lists.shape == (40, 24)
    assert sorted(sr.WIDTHS) == sorted({(d, 8) for d in (4, 252, 256, 260, 1020, 1024)} | {(20, q) for q in (4, 252, 256, 260, 512)}
                                       | {(1024, 512), (4, 4)})


@pytest.mark.parametrize("name", sr.case_names())
def test_case_is_well_conditioned_for_the_fp32_bounds(name):
    """The oracle in float32 on the CPU, against pool_ref: below a quarter of OUT_TOL['fp32'] and of grad_bound, elementwise."""
    c = sr.case(name)
    got, ref = _autograd(c, torch.float32), sr.reference(name)
    scale = max(1.0, float(np.abs(ref.out).max()))
    err = float(np.abs(got.out.numpy() - ref.out).max())
    print("%-16s out %.2e of %.2e" % (name, err, OUT_TOL["fp32"] * scale), end="")
    assert err < 0.25 * OUT_TOL["fp32"] * scale
    for f in ("dx", "dw", "db", "dq"):
        r = torch.from_numpy(getattr(ref, f))
        ratio = float(((getattr(got, f).double() - r).abs() / grad_bound(r)).max())
        print("  %s %.3f" % (f, ratio), end="")
        assert ratio < 0.25, (name, f, ratio)
    print()


@pytest.mark.parametrize("name", sr.case_names())
def test_case_is_well_conditioned_for_split_bf16_operands(name):
    """NRMS_PRECISION_BF16X3 is held to grad_bound as fp32 is, and its operands carry 16 significant bits whatever the kernel does:
    pool_ref with such operands and exact accumulation must stay below half of OUT_TOL['bf16x3'] and of grad_bound, which with
    the quarter the float32 oracle may take leaves a quarter of the bound to the kernel's own order of accumulation."""
    got, ref = sr.reference(name, "bf16x3"), sr.reference(name)
    scale = max(1.0, float(np.abs(ref.out).max()))
    err = float(np.abs(got.out - ref.out).max())
    print("%-16s out %.3f" % (name, err / (OUT_TOL["bf16x3"] * scale)), end="")
    assert err < 0.5 * OUT_TOL["bf16x3"] * scale
    for f in ("dx", "dw", "db", "dq"):
        r = torch.from_numpy(getattr(ref, f))
        ratio = float(((torch.from_numpy(getattr(got, f)) - r).abs() / grad_bound(r)).max())
        print("  %s %.3f" % (f, ratio), end="")
        assert ratio < 0.5, (name, f, ratio)
    print()


def test_the_projects_bf16_bars_cover_four_times_the_measured_deviation():
    """What NRMS_PRECISION_BF16 may cost comes from pool_ref alone: exact against bf16-rounded projection operands, times 4 for
    the order of accumulation.  BF16_SCORE_TOL / BF16_GRAD_RTOL (tests/test_hip_parity.py) cover it for every tensor, which is
    why tests/test_hip_segpool_edges.py uses them; the figures are in docs/EXPERIMENTS.md."""
    from tests.test_hip_segpool_edges import BF16_TOL
    dev = {n: sr.bf16_deviation(n) for n in sr.BF16_CASES}
    for n in sr.BF16_CASES:
        print("bf16 deviation %-15s" % n, "  ".join("%s %.2e" % (f, v) for f, v in dev[n].items()))
    recorded = {"out": 2.1e-3, "dx": 3.4e-3, "dw": 2.1e-2, "db": 4.3e-2, "dq": 1.45e-2}
    for f in ("out", "dx", "dw", "db", "dq"):
        need = 4.0 * max(dev[n][f] for n in sr.BF16_CASES)
        print("  %-3s 4 x worst = %.3e, bar %.1e" % (f, need, BF16_TOL[f]))
        assert need <= recorded[f] <= 1.1 * need and recorded[f] <= BF16_TOL[f], (f, need)
