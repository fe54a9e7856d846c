"""Argument checks of the node-feature keywords of ugs_sampler.wl (feature_labels, wl_hash(x= / node_labels=), WLVocab.ids): every
error is raised before any device work, so these run without a GPU.  Tensors "on another device" live on torch's meta device."""
import numpy as np
import pytest
import torch


def rows():
    nodes = torch.tensor([[0, 1, 2, -1], [3, -1, 4, 5]], dtype=torch.int64)
    ei = torch.tensor([[0, 1], [1, 0]], dtype=torch.int64)
    return nodes, ei, torch.tensor([0, 2, 2], dtype=torch.int64)


def calls():
    from ugs_sampler import wl
    table = wl.WLVocab({"0" * 32: 0}, "cuda:0")
    return [("wl_hash", lambda **kw: wl.wl_hash(*rows(), 3, **kw)), ("WLVocab.ids", lambda **kw: table.ids(*rows(), 3, **kw))]


def test_public_names():
    from ugs_sampler import wl
    assert "feature_labels" in wl.__all__ and callable(wl.feature_labels)


@pytest.mark.parametrize("which", [0, 1])
def test_label_keywords_are_checked_before_device_work(which):
    name, call = calls()[which]
    x = torch.eye(6, 3)
    labels = torch.arange(6, dtype=torch.int64)
    with pytest.raises(ValueError, match="mutually exclusive"):
        call(x=x, node_labels=labels)
    with pytest.raises(TypeError):
        call(x=x.to(torch.bfloat16))
    with pytest.raises(TypeError):
        call(x=torch.eye(6, 3, dtype=torch.complex64))
    with pytest.raises(TypeError):
        call(x=np.eye(6, 3, dtype=np.float32))
    with pytest.raises(ValueError):
        call(x=torch.tensor(1.0))
    with pytest.raises(TypeError):
        call(node_labels=labels.to(torch.int32))
    with pytest.raises(TypeError):
        call(node_labels=labels.tolist())
    with pytest.raises(ValueError):
        call(node_labels=labels.reshape(6, 1))
    with pytest.raises(ValueError):
        call(x=torch.empty((6, 3), device="meta"))
    with pytest.raises(ValueError):
        call(node_labels=torch.empty((6,), dtype=torch.int64, device="meta"))


def test_feature_labels_arguments():
    from ugs_sampler import wl
    with pytest.raises(TypeError):
        wl.feature_labels(torch.eye(4, 3, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        wl.feature_labels(np.eye(4, 3))
    with pytest.raises(ValueError):
        wl.feature_labels(torch.tensor(3))
    with pytest.raises(ValueError):
        wl.feature_labels(torch.empty((4, 3), device="meta"))
    with pytest.raises(ValueError):
        wl.feature_labels(torch.eye(4, 3), device="cpu")


def test_sampler_tensors_are_still_checked_first():
    from ugs_sampler import wl
    nodes, ei, ep = rows()
    with pytest.raises(TypeError):
        wl.wl_hash(nodes.to(torch.int32), ei, ep, 3, x=torch.eye(6, 3))
    with pytest.raises(ValueError):
        wl.wl_hash(nodes, ei, ep[:-1], 3, node_labels=torch.arange(6))
