"""ugs_collate_rows / ugs_collate_edges (csrc/ugs_collate.hip) against the collation law in plain numpy (tests/collate_law.py) and
against the CPU Collator, on synthetic per-rank results: every wire width, the block edges of both kernels, the rank layouts, the
steady state of one Collator over several steps, overflow at a multi-block size and the C entry point's refusals.  Every
comparison is exact integer equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import collate_law as law
import collate_run as run
from test_collate_law import WIRE, check_overflow_result, overflow_case

pytestmark = pytest.mark.gpu

CASES = law.all_cases()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def point_of(name, case, got, dst):
    """what the case is there for is really in it (and came out)"""
    group = name.split(":")[0]
    tot = sum(case.totals)
    if group == "rows_block":
        assert dst.rows_cap * case.k in (255, 256, 257, 511, 513) and dst.rows_cap == max(case.rows) and (got[0] == -1).any()
    elif group == "edges_block":
        want = tuple(int(x) for x in name.split(":")[1].split("-")[1:4])
        assert tuple(case.totals) == want and dst.eb == {"u8": 1, "i32": 4, "i64": 8}[name.split(":")[1].split("-")[0]]
        assert dst.edge_cap == max(want) + int(name.rsplit("+", 1)[1])
        if max(want) > 1024:
            assert tot > 1024 and dst.edge_cap > 1024
    elif group == "width":
        assert (got[0] == -1).any() or name.endswith("k256")
        parts = name.split(":")[1].split("-")
        if len(parts) == 3 and parts[0] in WIRE:
            assert [dst.nd, dst.ed, dst.sd] == [WIRE[w] for w in parts]
            if parts[1] == "u8":
                assert (got[1][:, :tot] == 199).any() and (got[1][:, :tot] >= 128).any() and case.k == 200 and case.rows == [3, 3]
            for arr, w in ((got[0], parts[0]), (got[1][:, :tot], parts[1]), (got[3][:tot], parts[2])):
                if w.endswith("64"):
                    assert all((arr == v).any() for v in (2 ** 31 - 1, 2 ** 31, 2 ** 40 + 7))
        elif name.endswith("2^31"):
            assert [dst.nd, dst.ed, dst.sd] == [torch.int64] * 3 and (got[0] == 2 ** 31 - 1).any()
        else:
            assert dst.ed == torch.int32 and case.k == 256 and (got[1][:, :tot] == 255).any()
    elif group == "failed_row":
        for row in (0, case.row_off[2] - 1, case.total_rows - 1):
            assert (got[0][row] == -1).all() and got[2][row] == got[2][row + 1]
    elif group == "layout" and case.world == 64:
        offs = np.concatenate([[0], np.cumsum(case.totals)])
        assert len(set(offs.tolist())) == 65                                        # every rank's offset differs from the one before
        for r in range(64):
            assert got[2][case.row_off[r]] == offs[r]
        assert got[2][-1] == offs[64]
    elif group == "no_edge":
        assert dst.edge_cap == 0 and case.k == 1 and not got[2].any() and got[2].shape == (case.total_rows + 1,)
    elif group == "empty_batch":
        assert got[0].shape == (0, case.k) and got[2].tolist() == [0]


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_collator_obeys_the_law(name):
    case, cap, junk = CASES[name]
    cap = run.edge_cap_of(case, cap)
    packers, msgs = run.pack_all(case, dev(), cap, junk)
    dst_gpu, dst_cpu = run.collator(case, 0, dev(), cap), run.collator(case, 0, "cpu", cap)
    run.deliver(dst_gpu, msgs)
    run.deliver(dst_cpu, msgs)
    got, ref = run.unpack_numpy(dst_gpu), run.unpack_numpy(dst_cpu)
    run.assert_law(got, case.expected(), name + " (HIP)")
    run.assert_law(ref, case.expected(), name + " (torch path)")
    tot = sum(case.totals)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[1][:, :tot], ref[1][:, :tot]) and np.array_equal(got[3][:tot], ref[3][:tot])
    assert not dst_gpu.overflowed() and not dst_cpu.overflowed() and not any(p.overflowed() for p in packers)
    assert int(dst_gpu.max_total.item()) == max(case.totals) == int(dst_cpu.max_total.item())
    point_of(name, case, got, dst_gpu)


def test_world_above_64_is_refused():
    with pytest.raises(RuntimeError):
        run.ud.Collator(130, 3, "global", 10, 10, 10, 4, dev(), world=65, rank=0)


@pytest.mark.parametrize("side_stream", [False, True])
def test_steady_state(side_stream):
    """one destination and one packer per rank, five steps whose totals grow and shrink: stale entries of a fuller step never show
    below a step's total, max_total keeps the maximum; the same with copies and unpack() issued on a side stream"""
    steps = law.steady_state_steps(21 + side_stream)
    cap = max(max(s.totals) for s in steps)
    assert cap == 2049 and [sum(s.totals) for s in steps] == [2400, 9, 0, 3074, 2010]
    dst, packers = run.collator(steps[0], 0, dev(), cap), None
    stream = torch.cuda.Stream(dev()) if side_stream else torch.cuda.current_stream(dev())
    torch.cuda.synchronize()
    for i, s in enumerate(steps):
        packers, msgs = run.pack_all(s, dev(), cap, packers=packers)
        stream.wait_stream(torch.cuda.current_stream(dev()))                        # the messages are packed on the current stream
        with torch.cuda.stream(stream):
            run.deliver(dst, msgs)
            out = dst.unpack()
        stream.synchronize()
        torch.cuda.current_stream(dev()).wait_stream(stream)                        # the next step's packing overwrites the messages
        run.assert_law([t.cpu().numpy() for t in out], s.expected(), f"step {i}")
    assert int(dst.max_total.item()) == 2049 and not dst.overflowed()


def test_overflow_at_multi_block_size():
    case = overflow_case()
    packers, msgs = run.pack_all(case, dev(), 1500)
    dst_gpu, dst_cpu = run.collator(case, 0, dev(), 1500), run.collator(case, 0, "cpu", 1500)
    guard = torch.full((64,), -12345, dtype=torch.int64, device=dev())              # allocated right behind the output buffers
    assert [p.overflowed() for p in packers] == [False, True, False]
    run.deliver(dst_gpu, msgs)
    run.deliver(dst_cpu, msgs)
    got, ref = run.unpack_numpy(dst_gpu), run.unpack_numpy(dst_cpu)
    torch.cuda.synchronize()
    check_overflow_result(dst_gpu, got, case)
    check_overflow_result(dst_cpu, ref, case)
    assert bool((guard == -12345).all())
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and int(dst_gpu.max_total.item()) == int(dst_cpu.max_total.item())
    assert np.array_equal(got[1][:, :1200], ref[1][:, :1200]) and np.array_equal(got[3][:1200], ref[3][:1200])
    # the entries the truncated rank did send, and the last rank's behind them, are at their places too
    _, eidx, _, esrc = case.expected()
    for lo, hi in ((1200, 2700), (2900, 3700)):
        assert np.array_equal(got[1][:, lo:hi], eidx[:, lo:hi]) and np.array_equal(got[3][lo:hi], esrc[lo:hi])


def test_refusals_leave_the_outputs_alone_and_the_library_usable():
    """argument errors of ugs_collate_unpack: nonzero status and a message before any launch, nothing written; a good call after"""
    from ugs_sampler._lib import lib
    case = law.make_case(np.random.default_rng(31), 2, (3, 2), 4, (20, 9), 3000, 3000, 9000, "global")
    _, msgs = run.pack_all(case, dev(), 20)
    dst = run.collator(case, 0, dev(), 20)
    run.deliver(dst, msgs)
    outs = (dst.out_nodes, dst._eidx_buf, dst.out_eptr, dst._esrc_buf, dst.max_total)
    for t in outs:
        t.fill_(-777)
    torch.cuda.synchronize()

    def call(world=2, row_off=(0, 3, 5), nb=4, eb=4, sb=4, rows_cap=3, nodes_ptr=None):
        ro = (C.c_int64 * len(row_off))(*row_off)
        return lib.ugs_collate_unpack(dst.inbox.data_ptr(), world, ro, 4, nb, eb, sb, rows_cap, 20, dst.out_nodes.data_ptr() if nodes_ptr is None else nodes_ptr,
                                      dst.out_eidx.data_ptr(), dst.out_eidx.stride(0), dst.out_eptr.data_ptr(), dst.out_esrc.data_ptr(),
                                      dst.max_total.data_ptr(), torch.cuda.current_stream(dev()).cuda_stream)

    assert (dst.nb, dst.eb, dst.sb, dst.rows_cap) == (4, 4, 4, 3)
    bad = {"world 0": dict(world=0), "world 65": dict(world=65, row_off=tuple(range(66))), "node width 1": dict(nb=1), "edge_index width 2": dict(eb=2),
           "edge_src width 1": dict(sb=1), "rows above rows_cap": dict(rows_cap=2), "decreasing row_off": dict(row_off=(0, 3, 2)),
           "null nodes with rows": dict(nodes_ptr=0)}
    for what, kw in bad.items():
        assert call(**kw) != 0, what
        assert (lib.ugs_last_error() or b"").decode(), what
        torch.cuda.synchronize()
        assert all(bool((t == -777).all()) for t in outs), what
    dst.max_total.zero_()
    run.assert_law(run.unpack_numpy(dst), case.expected(), "after the refusals")
    assert int(dst.max_total.item()) == 20
    assert call() == 0
