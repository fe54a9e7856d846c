"""Drives ugs_sampler.distributed.Collator over the synthetic cases of tests/collate_law.py without a process group: every rank's
locals are packed by a Collator of that rank, the messages are placed in a destination's inbox by hand, the destination unpacks."""
import numpy as np
import torch

from ugs_sampler import distributed as ud


def collator(case, rank, device, edge_cap):
    return ud.Collator(case.total_rows, case.k, case.mode, case.node_bound, case.edge_id_bound, case.col_bound, edge_cap, device, dst=0,
                       world=case.world, rank=rank, row_off=case.row_off)


def edge_cap_of(case, edge_cap):
    return max(case.totals) if edge_cap is None else int(edge_cap)


def to_device(local, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in local)


def pack_all(case, device, edge_cap, junk=None, packers=None):
    """(packers, messages): one packer per rank (made here unless given), each rank's locals packed on `device`"""
    if packers is None:
        packers = [collator(case, r, device, edge_cap) for r in range(case.world)]
    locals_ = case.locals if junk is None else case.padded(edge_cap, junk)
    return packers, [p.pack(to_device(l, device)) for p, l in zip(packers, locals_)]


def deliver(dst, msgs):
    for r, m in enumerate(msgs):
        dst.inbox[r].copy_(m.to(dst.inbox.device))


def unpack_numpy(dst):
    return [t.cpu().numpy() for t in dst.unpack()]


def assert_law(got, want, what):
    """exact equality of an unpacked batch (capacity-sized edge buffers) to the law's (exact-size) tensors"""
    nodes, eidx, eptr, esrc = want
    tot = int(eptr[-1])
    assert got[0].shape == nodes.shape and got[0].dtype == np.int64, what
    assert np.array_equal(got[0], nodes), f"{what}: nodes"
    assert np.array_equal(got[2], eptr), f"{what}: edge_ptr"
    assert got[1].shape[1] >= tot and got[3].shape[0] >= tot, what
    assert np.array_equal(got[1][:, :tot], eidx), f"{what}: edge_index"
    assert np.array_equal(got[3][:tot], esrc), f"{what}: edge_src"
