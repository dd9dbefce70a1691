"""Helpers of the "graphed == eager" tests (tests/test_gpu_graphed_classifiers.py and the graphed legs of the per-kernel
files).  A comparison of a hipGraph replay with the eager loop proves something only if a graph was really recorded and
replayed: engine.DDragueSolver.run(use_graph=True) answers a failed capture with a RuntimeWarning, `_graph = False` and the
eager loop, which every "equal bits" assertion then passes trivially.  So every such test

  * runs its graphed leg inside `no_capture_fallback()` (the warning of the fall-back is an error there), and
  * ends with `assert_graph_used(obj)`: the object holds a torch.cuda.CUDAGraph, not None, not False.

`same_state` is the comparison (bytes, not values: -0.0 / +0.0 and NaN payloads count) and names what differs;
`library_free` counts the library calls a classifier still makes, which is the precondition under which the eager loop is
its own bitwise reference.  Plain module: no fixtures, no pytest settings; the CPU checks are in test_graph_tools_cpu.py."""
import contextlib
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F


def assert_graph_used(obj):
    """`obj` (an engine.DDragueSolver or an engine.DictionaryLearner) has recorded a hipGraph.  The solver keeps the graph
    itself in `_graph` (None: never tried, False: the capture failed and the eager loop ran); the learner keeps a tuple
    whose first element is the graph."""
    g = getattr(obj, "_graph", None)
    if isinstance(g, tuple):
        assert len(g) > 0 and isinstance(g[0], torch.cuda.CUDAGraph), \
            "%s._graph[0] is %r, not a recorded graph" % (type(obj).__name__, g[0] if g else None)
        return
    assert g is not None, "%s recorded no graph (_graph is None): its steps ran eagerly" % type(obj).__name__
    assert g is not False, "%s fell back to the eager loop (_graph is False): the capture failed" % type(obj).__name__
    assert isinstance(g, torch.cuda.CUDAGraph), "%s._graph is %r, not a recorded graph" % (type(obj).__name__, g)


@contextlib.contextmanager
def no_capture_fallback():
    """Inside, a RuntimeWarning is an error: the solver's fall-back to the eager loop after a failed capture raises
    instead of passing for a graphed run.  The filters in force outside are restored on exit."""
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        yield


def _bytes(t):
    t = t.detach()
    if not t.is_contiguous():
        t = t.contiguous()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1).to(torch.uint8)


def first_difference(a, b, names):
    """None if every named tensor attribute (or mapping entry) of a and b holds the same bytes, else a sentence that names
    the first one that does not, with the number of differing elements."""
    get = (lambda o, n: o[n]) if isinstance(a, dict) else getattr
    for name in names:
        x, y = get(a, name), get(b, name)
        if x.dtype != y.dtype or tuple(x.shape) != tuple(y.shape):
            return "%s: %s %s against %s %s" % (name, x.dtype, tuple(x.shape), y.dtype, tuple(y.shape))
        bx, by = _bytes(x), _bytes(y.to(x.device))
        if not torch.equal(bx, by):
            size = max(1, x.element_size())
            wrong = int((bx != by).reshape(-1, size).any(dim=1).sum())
            return "%s differs in %d of %d elements" % (name, wrong, x.numel())
    return None


def same_state(a, b, names):
    """The named tensors of a and b are equal byte for byte (compared through a uint8 view); the assertion message names
    the first that differs and how many of its elements do."""
    diff = first_difference(a, b, names)
    assert diff is None, diff


class LibraryCalls:
    """Counts F.conv2d, F.batch_norm, F.linear, F.adaptive_avg_pool2d and nn.Conv2d.forward while it is in force (the idea
    of `_Calls` in test_gpu_head.py, without a monkeypatch fixture: it patches on entry and restores on exit)."""
    FUNCTIONS = ("conv2d", "batch_norm", "linear", "adaptive_avg_pool2d")

    def __init__(self):
        self.n = dict.fromkeys(self.FUNCTIONS + ("Conv2d.forward",), 0)
        self._saved = []

    def _counting(self, name, real):
        def call(*args, **kw):
            self.n[name] += 1
            return real(*args, **kw)
        return call

    def __enter__(self):
        for name in self.FUNCTIONS:
            self._saved.append((F, name, getattr(F, name)))
            setattr(F, name, self._counting(name, getattr(F, name)))
        self._saved.append((nn.Conv2d, "forward", nn.Conv2d.forward))
        nn.Conv2d.forward = self._counting("Conv2d.forward", nn.Conv2d.forward)
        return self

    def __exit__(self, *exc):
        for owner, name, real in reversed(self._saved):
            setattr(owner, name, real)
        self._saved = []


def library_free(model, x, claims=()):
    """One forward + input gradient of `model` at `x` with the library entry points counted; returns the counts as a dict
    after asserting that no convolution and no BatchNorm was called, nor any of `claims` (names out of "linear",
    "adaptive_avg_pool2d": what the build says it has replaced as well).  Patches and restores the functions itself."""
    x = x.detach().clone().requires_grad_(True)
    with LibraryCalls() as calls:
        out = model(x)
        (g,) = torch.autograd.grad(out.float().square().sum(), x)
    assert g.shape == x.shape
    n = dict(calls.n)
    for name in ("conv2d", "batch_norm", "Conv2d.forward") + tuple(claims):
        assert n[name] == 0, "library call left in forward + input gradient: %s x %d (%r)" % (name, n[name], n)
    return n
