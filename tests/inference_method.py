"""What the host tests assert of a model's ``.inference``: it IS ``inference.layerwise_inference`` of that model.  Without
a device that shows in what the two raise -- the same exception type and the same message for the same bad argument,
and, with every argument in order, the error of the missing device that ``SAGE.inference`` gives."""
import pytest
import torch


def _raised(call):
    with pytest.raises(Exception) as info:
        call()
    return type(info.value), str(info.value)


def assert_method_is_the_function(model, x, rowptr, col, **good):
    """``good``: keywords the model's valid call needs besides the graph (GCN: ``edge_weight``)"""
    from salient_plusplus_amd.inference import layerwise_inference
    was_training = model.training
    bad_calls = [((x, rowptr, col), dict(act_dtype=torch.float16)),
                 ((x, rowptr, col), dict(rows_per_slab=0)),
                 ((x, rowptr, col), dict(nodes=torch.tensor([0.5]))),
                 ((x, rowptr[:-1], col), {}),                 # a malformed graph: one row per node
                 ((x, rowptr.to(torch.int32), col), {})]
    kinds = []
    for args, kw in bad_calls:
        method = _raised(lambda: model.inference(*args, **good, **kw))
        assert method == _raised(lambda: layerwise_inference(model, *args, **good, **kw)), (method, kw)
        assert method[0] is ValueError and method[1].startswith("layerwise_inference: "), method
        kinds.append(method[1])
    assert "act_dtype" in kinds[0] and "rows_per_slab" in kinds[1] and "nodes" in kinds[2] and \
        "one row per node" in kinds[3] and "rowptr" in kinds[4]
    assert model.training == was_training                     # a refused call leaves the mode alone
    if not torch.cuda.is_available():                         # no CPU fallback: valid arguments need the device
        from salient_plusplus_amd import _native as nat
        from salient_plusplus_amd.models import SAGE
        sage = SAGE(x.size(1), 4, 2, 2)
        want = _raised(lambda: sage.inference(x, rowptr, col))
        assert want[0] is nat.SppError
        assert _raised(lambda: model.inference(x, rowptr, col, **good)) == want
        assert model.training == was_training


def assert_method_equals_function(model, x, rowptr, col, nodes, act_dtype, **kw):
    """on the device: ``model.inference`` returns the bits of ``layerwise_inference`` of the same call, for every node and
    for ``nodes``, and leaves the model's mode alone"""
    from salient_plusplus_amd.inference import layerwise_inference
    was_training = model.training
    for select in ({}, {"nodes": nodes}):
        want = layerwise_inference(model, x, rowptr, col, act_dtype=act_dtype, **select, **kw)
        got = model.inference(x, rowptr, col, act_dtype=act_dtype, **select, **kw)
        rows = nodes.numel() if select else x.size(0)
        assert got.dtype == torch.float32 and got.size(0) == rows and not got.requires_grad
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want), sorted(select)
        assert model.training == was_training
    return got
