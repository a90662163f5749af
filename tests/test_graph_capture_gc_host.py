"""nerf.graph.capture_graph keeps Python's cyclic collector out of a graph
capture: dead cycles are collected before it begins, the collector is off
inside and back on afterwards (also when the body raises).  torch.cuda.graph
is replaced by a recorder, so no device is needed."""
import contextlib
import gc
import weakref

import pytest


class _Node:
    pass


def test_capture_graph_collects_before_and_disables_gc_inside(monkeypatch):
    import torch
    from nerf import graph as ng
    seen = {}

    @contextlib.contextmanager
    def fake_graph(graph, **kwargs):
        seen["args"] = (graph, kwargs)
        seen["gc_inside"] = gc.isenabled()
        seen["cycle_alive_at_begin"] = ref() is not None
        yield

    monkeypatch.setattr(torch.cuda, "graph", fake_graph)
    gc.collect()
    gc.disable()            # build a dead cycle that only the collector frees
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    ref = weakref.ref(a)
    del a, b
    gc.enable()
    assert ref() is not None
    with ng.capture_graph("g", stream="s", pool="p"):
        assert not gc.isenabled()
    assert seen["args"] == ("g", {"stream": "s", "pool": "p"})
    assert seen["gc_inside"] is False and seen["cycle_alive_at_begin"] is False
    assert gc.isenabled()
    with pytest.raises(ValueError):
        with ng.capture_graph("g"):
            raise ValueError("body")
    assert gc.isenabled()
    gc.disable()            # a caller that runs with the collector off keeps it off
    try:
        with ng.capture_graph("g"):
            pass
        assert not gc.isenabled()
    finally:
        gc.enable()
