"""CPU checks of tests/graph_tools.py with stand-in objects: the helpers decide whether a "graphed == eager" test proves
anything, so each of them is shown to refuse what it must refuse."""
import contextlib
import gc
import warnings
import weakref

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import graph_tools as G


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _FakeGraph:
    pass


def test_assert_graph_used_rejects_none_false_and_anything_that_is_no_graph(monkeypatch):
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    G.assert_graph_used(_Obj(_graph=_FakeGraph()))                                  # a solver that recorded
    G.assert_graph_used(_Obj(_graph=(_FakeGraph(), None, None, None, None, 8, None)))   # a learner that recorded
    with pytest.raises(AssertionError, match="is None"):
        G.assert_graph_used(_Obj(_graph=None))
    with pytest.raises(AssertionError, match="fell back"):
        G.assert_graph_used(_Obj(_graph=False))                # what `_graph is not None` used to let through
    with pytest.raises(AssertionError):
        G.assert_graph_used(_Obj())
    with pytest.raises(AssertionError):
        G.assert_graph_used(_Obj(_graph=True))
    with pytest.raises(AssertionError):
        G.assert_graph_used(_Obj(_graph=object()))
    with pytest.raises(AssertionError):
        G.assert_graph_used(_Obj(_graph=(None, 1, 2)))
    with pytest.raises(AssertionError):
        G.assert_graph_used(_Obj(_graph=(False,)))
    with pytest.raises(AssertionError):
        G.assert_graph_used(_Obj(_graph=()))


def test_no_capture_fallback_turns_the_warning_into_an_error_and_restores_the_filters():
    before = list(warnings.filters)
    with pytest.raises(RuntimeWarning, match="capture failed"):
        with G.no_capture_fallback():
            warnings.warn("capture failed; running the eager loop instead", RuntimeWarning)
    with G.no_capture_fallback():
        with warnings.catch_warnings(record=True) as seen:     # other categories stay warnings
            warnings.simplefilter("always")
            warnings.warn("something else", UserWarning)
        assert len(seen) == 1
    assert list(warnings.filters) == before
    with warnings.catch_warnings(record=True) as seen:         # outside, the RuntimeWarning is a warning again
        warnings.simplefilter("always")
        warnings.warn("capture failed", RuntimeWarning)
    assert len(seen) == 1 and seen[0].category is RuntimeWarning


def test_same_state_names_the_first_tensor_that_differs():
    g = torch.Generator().manual_seed(0)
    a = _Obj(d=torch.rand(3, 4, generator=g), v=torch.rand(5, generator=g), m=torch.zeros(2, dtype=torch.bfloat16))
    b = _Obj(d=a.d.clone(), v=a.v.clone(), m=a.m.clone())
    G.same_state(a, b, ("d", "v", "m"))
    b.v[1] += 1.0
    b.v[3] += 1.0
    b.m[0] = 1.0
    with pytest.raises(AssertionError, match=r"^v differs in 2 of 5 elements$"):
        G.same_state(a, b, ("d", "v", "m"))
    with pytest.raises(AssertionError, match=r"^m differs in 1 of 2 elements$"):
        G.same_state(a, b, ("d", "m", "v"))
    G.same_state(a, b, ("d",))
    # bytes, not values: the two zeros are different states, equal NaNs are the same state
    z = _Obj(d=torch.tensor([0.0, float("nan")]))
    w = _Obj(d=torch.tensor([-0.0, float("nan")]))
    assert torch.equal(z.d[:1], w.d[:1])
    with pytest.raises(AssertionError, match="d differs in 1 of 2 elements"):
        G.same_state(z, w, ("d",))
    G.same_state(z, _Obj(d=z.d.clone()), ("d",))
    # dtype and shape are part of the state; mappings are compared by key
    with pytest.raises(AssertionError, match="d: "):
        G.same_state(_Obj(d=torch.zeros(2)), _Obj(d=torch.zeros(2, dtype=torch.float64)), ("d",))
    with pytest.raises(AssertionError, match="d: "):
        G.same_state(_Obj(d=torch.zeros(2)), _Obj(d=torch.zeros(3)), ("d",))
    G.same_state({"z": torch.ones(2, 2).t()}, {"z": torch.ones(2, 2)}, ("z",))
    with pytest.raises(AssertionError, match="z differs in 4 of 4"):
        G.same_state({"z": torch.ones(2, 2)}, {"z": torch.zeros(2, 2)}, ("z",))


class _OwnLike(nn.Module):
    """No library convolution or BatchNorm: an elementwise stand-in with a Linear head."""

    def __init__(self, head=True):
        super().__init__()
        self.fc = nn.Linear(12, 3) if head else None

    def forward(self, x):
        h = torch.relu(x * 2.0 - 0.5).flatten(1)
        return self.fc(h) if self.fc is not None else h[:, :3]


class _LibraryNet(nn.Sequential):
    def __init__(self, bn):
        layers = [nn.Conv2d(3, 4, 3, padding=1)] + ([nn.BatchNorm2d(4)] if bn else []) + \
                 [nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(4, 3)]
        super().__init__(*layers)


def test_library_free_counts_patches_and_restores():
    real = (F.conv2d, F.batch_norm, F.linear, F.adaptive_avg_pool2d, nn.Conv2d.forward)
    x = torch.rand(2, 3, 2, 2)
    n = G.library_free(_OwnLike().eval(), x)
    assert n == {"conv2d": 0, "batch_norm": 0, "linear": 1, "adaptive_avg_pool2d": 0, "Conv2d.forward": 0}
    with pytest.raises(AssertionError, match="linear x 1"):
        G.library_free(_OwnLike().eval(), x, claims=("linear", "adaptive_avg_pool2d"))
    G.library_free(_OwnLike(head=False).eval(), x, claims=("linear", "adaptive_avg_pool2d"))
    with pytest.raises(AssertionError, match="conv2d x 1"):
        G.library_free(_LibraryNet(bn=False).eval(), x)
    with pytest.raises(AssertionError, match="library call left"):
        G.library_free(_LibraryNet(bn=True).eval(), x)

    class OnlyBatchNorm(nn.Module):
        def forward(self, x):
            return F.batch_norm(x, torch.zeros(3), torch.ones(3)).flatten(1)
    with pytest.raises(AssertionError, match="batch_norm x 1"):
        G.library_free(OnlyBatchNorm(), x)
    # restored after success and after failure alike, and the input was not touched
    assert (F.conv2d, F.batch_norm, F.linear, F.adaptive_avg_pool2d, nn.Conv2d.forward) == real
    assert not x.requires_grad
    with G.LibraryCalls() as calls:
        _LibraryNet(bn=True).eval()(x)
    assert calls.n == {"conv2d": 1, "batch_norm": 1, "linear": 1, "adaptive_avg_pool2d": 1, "Conv2d.forward": 1}
    assert (F.conv2d, F.batch_norm, F.linear, F.adaptive_avg_pool2d, nn.Conv2d.forward) == real


class _Cycle:
    def __init__(self):
        self.me = self


def test_capture_graph_collects_first_and_holds_the_collector_off(monkeypatch):
    """engine.capture_graph around a stand-in for torch.cuda.graph: a dead cycle is gone when the capture begins, no
    collection runs while it lasts (a cycle that dies inside survives allocations that would otherwise trigger one), and
    the collector is left as it was found, after an exception too."""
    from dl_attack_on_imagenet_amd import engine
    seen = []

    @contextlib.contextmanager
    def stand_in(graph):
        seen.append(("begin", graph, ref() is None, gc.isenabled()))
        yield
        seen.append(("end", graph, inner() is None, gc.isenabled()))

    monkeypatch.setattr(torch.cuda, "graph", stand_in)
    was_enabled = gc.isenabled()
    gc.disable()                                                          # nothing but capture_graph collects `ref`
    ref = weakref.ref(_Cycle())
    assert ref() is not None
    gc.enable()
    try:
        with engine.capture_graph("g") as g:
            assert g == "g" and not gc.isenabled()
            inner = weakref.ref(_Cycle())
            junk = [[] for _ in range(20000)]                             # far beyond the collector's first threshold
            assert inner() is not None and len(junk) == 20000
        assert gc.isenabled()
        assert seen == [("begin", "g", True, False), ("end", "g", False, False)]
        gc.collect()
        assert inner() is None
        with pytest.raises(ValueError):
            with engine.capture_graph("h"):
                raise ValueError("inside")
        assert gc.isenabled()
        gc.disable()                                                      # found off: left off
        with engine.capture_graph("i"):
            pass
        assert not gc.isenabled()
    finally:
        gc.enable() if was_enabled else gc.disable()
