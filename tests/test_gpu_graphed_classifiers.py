"""GPU: hipGraph capture and replay of the attack's own loops with the kernel-built classifiers inside, against the eager
loops, bit for bit.  This is the path main.py takes by default (--graph 1).  No tolerance anywhere: an eager and a graphed
run issue the same launches on the same operands, so the claim is equality of bytes (graph_tools.same_state).

Per build (bf16, channels_last, 10 classes, from a seed; the smallest images at which every stride-2 kernel still gets an
even, covered input: 64 -> 16 -> 8 -> 4 -> 2):

  precondition  a condition on the reference alone, not a measurement: forward + input gradient call no library
                convolution and no BatchNorm (nor what else the build claims to have replaced), and two eager
                engine.input_gradient calls on the same input return the same bits.  Only then is the eager loop a bitwise
                reference; a build that fails it is a finding and gets no tolerance.
  learner       engine.DictionaryLearner.step against step_graphed from one state, 8 steps over minibatches whose contents
                change while their size stays, labels recomputed and cached: loss and fooled count at every step, d, v and
                the four moments at the end, the step counters, and a graph really recorded.  On resnet18 and densenet121
                also a ragged batch (falls back to the eager step) and the 8-bit store as `x`.
  solver        engine.DDragueSolver.run(12) against run(12, use_graph=True): z, m, s, result(), iters; then reset() with a
                second batch on the graphed solver (the recorded graph serves it) against a fresh eager solver.
  ADIL          on resnet18: ADIL(method="gd") with and without use_graph writes the same dictionary file.

Two tests show that the comparison can fail (a host value baked into the recording; a capture that falls back), neither by
making the GPU misbehave.  The "inference" DenseNet row keeps norm5 as a library BatchNorm outside engine.precise_head (that
is what "inference" means), so its plain call does not meet the precondition: it has the solver leg, whose calls run inside
precise_head, and the DenseNet learner legs run on the row whose head is always on."""
import gc
import weakref

import pytest
import torch

from graph_tools import assert_graph_used, first_difference, library_free, no_capture_fallback, same_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF16 = torch.bfloat16
ATOMS, CLASSES = 6, 10
EPS_LEARNER, EPS_SOLVER = 0.3, 0.1
LEARNER_STATE = ("d", "v", "m_d", "s_d", "m_v", "s_v")
SOLVER_STATE = ("z", "m", "s")

RESNET = dict(fuse_bn_act=True, fuse_stem=True, own_strided_conv=True)            # chain joins are on by default
MOBILENET = dict(own_depthwise=True, own_pointwise=True, own_first_conv=True, head_fp32=True)
DENSE5 = dict(own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True, own_dense_transition=True,
              own_dense_stem=True)

# id: (network, keywords, images per batch, image size, what the plain call claims besides convolution and BatchNorm,
#      whether the row has an fp32 head that only engine.precise_head switches on)
HEAD_CALLS = ("linear", "adaptive_avg_pool2d")
BUILDS = {
    "resnet50": ("resnet50", RESNET, 8, 64, (), False),
    "resnet50-head": ("resnet50", dict(RESNET, head_fp32="inference"), 8, 64, (), True),
    "resnet18": ("resnet18", RESNET, 8, 64, (), False),
    "mobilenet": ("mobilenet", MOBILENET, 8, 64, HEAD_CALLS, False),
    "densenet121": ("densenet121", dict(DENSE5, own_dense_head=True), 4, 64, HEAD_CALLS, False),
    "densenet121-head": ("densenet121", dict(DENSE5, own_dense_head="inference"), 4, 64, (), True),
    "vit-small": (None, None, 8, 32, (), False),
}
ALL = list(BUILDS)
LEARNER_BUILDS = [b for b in ALL if b != "densenet121-head"]        # see the module docstring
_SHARED = {}


@pytest.fixture(autouse=True)
def collect_dead_cycles_after_each_test():
    """A pytest.raises block closes a cycle (exception -> traceback -> frame -> the learner or solver in it), so several
    tests here leave dead cycles that hold a recorded graph, its memory pool and pinned ring.  They are collected when the
    test is over, outside any capture: a collection that falls into a later capture would run those destructors inside it
    (engine.capture_graph guards the product's captures; the per-kernel files call torch.cuda.graph themselves)."""
    yield
    gc.collect()


def shared(key, make):
    """Computed once and left unchanged."""
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def engine():
    from dl_attack_on_imagenet_amd import engine as e
    return e


def classifier(build):
    def make():
        name, kw = BUILDS[build][:2]
        if name is None:
            from test_gpu_attention import _small_vit
            return _small_vit(BF16, True)
        from dl_attack_on_imagenet_amd import zoo
        return zoo.build_classifier(name, num_classes=CLASSES, seed=7, device=DEV, dtype=BF16, channels_last=True, **kw)
    return shared(("net", build), make)


def byte_images(n, size, seed):
    """n images of 8-bit values u/255 (so that the same rows can live in an 8-bit store), fp32 on the host."""
    u = torch.randint(0, 256, (n, 3, size, size), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return u, u.float().div(255)


def dictionary(build, seed=3):
    size = BUILDS[build][3]
    return shared(("d", build, seed), lambda: (-1 + 2 * torch.rand(3, size, size, ATOMS,
                                                                   generator=torch.Generator().manual_seed(seed))).to(DEV))


class _Items(torch.utils.data.Dataset):
    """(image, label) items with the `indexed` protocol of the learners' datasets."""

    def __init__(self, images):
        self.images, self.indexed = images, False

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return (i, self.images[i], 0) if self.indexed else (self.images[i], 0)


def schedule(n, batch, steps, seed, ragged=0):
    """`steps` index batches out of range(n): a fresh permutation per epoch, cut into batches of `batch`; with `ragged`
    every fourth batch has only that many rows (the recording is made at the third call, at the full size)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    while len(out) < steps:
        perm = torch.randperm(n, generator=g).tolist()
        at = 0
        while at + batch <= n and len(out) < steps:
            size = ragged if (ragged and len(out) % 4 == 3) else batch
            out.append(perm[at:at + size])
            at += size
    return out


# ------------------------------------------------------------------------------------------------------ precondition
def _gradient_twice(model, x, labels):
    e = engine()
    a = e.input_gradient(model, x, labels, "logits", -1.0, 50.0, "sum")
    b = e.input_gradient(model, x, labels, "logits", -1.0, 50.0, "sum")
    names = ("logits", "loss", "gradient")
    same_state(dict(zip(names, a)), dict(zip(names, b)), names)
    assert bool(torch.isfinite(a[0].float()).all()) and float(a[2].float().abs().max()) > 0


@pytest.mark.parametrize("build", ALL)
def test_precondition_the_eager_reference_is_library_free_and_repeatable(build):
    e = engine()
    model = classifier(build)
    _, _, batch, size, claims, inference = BUILDS[build]
    x = byte_images(batch, size, 21)[1].to(DEV).to(BF16)
    labels = e.predict(model, x)
    if build in LEARNER_BUILDS:                                        # the plain call: what the learner's step makes
        print(build, "plain call:", library_free(model, x, claims))
        _gradient_twice(model, x, labels)
    if inference:                                                      # inside precise_head: what the solver's iteration makes
        with e.precise_head(model):
            print(build, "inside precise_head:", library_free(model, x, HEAD_CALLS if build.startswith("densenet") else ()))
            assert model(x).dtype == torch.float32
            _gradient_twice(model, x, labels)
        assert model(x).dtype == BF16


# ----------------------------------------------------------------------------------------------------------- learner
def _learner_pair(build, n, seed):
    e = engine()
    from dl_attack_on_imagenet_amd import ops
    g = torch.Generator().manual_seed(seed)
    v0 = ops.l1ball_project_(torch.rand(n, ATOMS, generator=g).to(DEV), EPS_LEARNER)
    d0 = dictionary(build)
    make = lambda: e.DictionaryLearner(d0.clone(), v0.clone(), EPS_LEARNER, 0.01, "logits")
    return make(), make(), d0


def _run_pair(model, a, b, batches, x_of, full_labels):
    """`a` steps eagerly, `b` through step_graphed, on the same batches; loss and fooled count equal at every step."""
    losses = []
    with no_capture_fallback():
        for step, idx in enumerate(batches):
            index = torch.tensor(idx, device=DEV)
            lab = full_labels[index] if full_labels is not None else None
            la, fa = a.step(model, x_of(index), index, lab)
            lb, fb = b.step_graphed(model, x_of(index), index, lab)
            diff = first_difference({"loss": la, "fooled": fa}, {"loss": lb, "fooled": fb}, ("loss", "fooled"))
            assert diff is None, "step %d: %s (%r against %r)" % (step, diff, float(la), float(lb))
            losses.append(float(la))
    return losses


def _check_learners(a, b, d0, steps, losses):
    same_state(a, b, LEARNER_STATE)
    assert a.sched_d.t == b.sched_d.t == steps and a.sched_v.t == b.sched_v.t == steps
    assert_graph_used(b)
    assert a._graph is None
    assert all(x == x and abs(x) < float("inf") for x in losses) and not torch.equal(a.d, d0)     # not a vacuous run


@pytest.mark.parametrize("labels", ["recomputed", "cached"])
@pytest.mark.parametrize("build", LEARNER_BUILDS)
def test_graphed_learner_step_equals_the_eager_step(build, labels):
    e = engine()
    model = classifier(build)
    batch, size = BUILDS[build][2:4]
    n = 3 * batch
    images = byte_images(n, size, 31)[1].to(DEV).to(BF16)
    full = e.predict(model, images) if labels == "cached" else None
    a, b, d0 = _learner_pair(build, n, 41)
    batches = schedule(n, batch, 8, 51)
    assert len({tuple(sorted(i)) for i in batches}) > 3                 # the contents change, the size does not
    losses = _run_pair(model, a, b, batches, lambda index: images[index].contiguous(), full)
    _check_learners(a, b, d0, 8, losses)
    assert b._graph[5] == batch and (b._graph[6] is None) == (full is None)


@pytest.mark.parametrize("leg", ["ragged", "store"])
@pytest.mark.parametrize("build", ["resnet18", "densenet121"])
def test_graphed_learner_ragged_batch_and_byte_store(build, leg):
    """ragged: every fourth batch is smaller — step_graphed falls back to the eager step for it and replays the recording
    for the others.  store: `x` is a loader.ResidentImages(dtype=torch.uint8); the recording holds the store's pointer and
    takes the rows from its static index buffer, the labels once recomputed (gather + forward inside the recording) and once
    cached."""
    e = engine()
    model = classifier(build)
    batch, size = BUILDS[build][2:4]
    short = batch // 2 + 1                                             # 5 of 8, 3 of 4
    n = 3 * batch + short
    u, f = byte_images(n, size, 33)
    if leg == "ragged":
        images = f.to(DEV).to(BF16)
        a, b, d0 = _learner_pair(build, n, 43)
        batches = schedule(n, batch, 8, 53, ragged=short)
        assert [len(i) for i in batches] == [batch, batch, batch, short] * 2
        losses = _run_pair(model, a, b, batches, lambda index: images[index].contiguous(), None)
        _check_learners(a, b, d0, 8, losses)
        assert b._graph[5] == batch
        return
    from dl_attack_on_imagenet_amd.loader import ResidentImages
    store = ResidentImages(_Items(u), DEV, torch.uint8, stream_dtype=BF16)
    assert store.is_bytes and store.images.dtype == torch.uint8 and torch.equal(store.images.cpu(), u)
    for cached in (False, True):
        full = e.predict(model, store.gather(torch.arange(n, device=DEV))) if cached else None
        a, b, d0 = _learner_pair(build, n, 45)
        losses = _run_pair(model, a, b, schedule(n, batch, 8, 55), lambda index: store, full)
        _check_learners(a, b, d0, 8, losses)
        assert b._graph[1] is store


# ------------------------------------------------------------------------------------------------------------ solver
def _head_counter(model):
    (head,) = [m.head32 for m in model.modules() if getattr(m, "head32", None) is not None]
    calls = {"n": 0}
    return calls, head.register_forward_hook(lambda *a: calls.__setitem__("n", calls["n"] + 1))


def _same_solvers(eager, graphed, steps):
    same_state(eager, graphed, SOLVER_STATE)
    names = ("adversarial images", "codes")
    same_state(dict(zip(names, eager.result())), dict(zip(names, graphed.result())), names)
    assert eager.iters == graphed.iters == steps


@pytest.mark.parametrize("build", ALL)
def test_graphed_solver_equals_the_eager_loop_and_serves_the_next_batch(build):
    e = engine()
    model = classifier(build)
    batch, size, _, inference = BUILDS[build][2:]
    images = byte_images(2 * batch, size, 35)[1].to(DEV).to(BF16)
    first, second = images[:batch].contiguous(), images[batch:].contiguous()
    d = dictionary(build, 5)
    pinv = e.PseudoInverse(d)
    solver = lambda x: e.DDragueSolver(model, x, d, EPS_SOLVER, "logits", pinv=pinv)
    calls, hook = _head_counter(model) if inference else ({"n": 0}, None)
    try:
        eager = solver(first).run(12)
        if inference:
            assert calls["n"] == 12                                     # once per eager iteration
        with no_capture_fallback():
            before = calls["n"]
            graphed = solver(first).run(12, use_graph=True)
        assert_graph_used(graphed)
        if inference:
            # three eager iterations and the three that are recorded pass through the Python module; the replays are those
            # recorded launches, so the fp32 head is in every replayed iteration: the bits below would differ otherwise
            assert calls["n"] == before + 6
            assert all(not m.head32_on for m in model.modules() if hasattr(m, "head32_on"))
        _same_solvers(eager, graphed, 12)
        assert bool(torch.isfinite(eager.z).all()) and float(eager.z.abs().max()) > 0
        assert bool((eager.result()[0] != first.clamp(0, 1)).any())    # not a vacuous run
        # the next batch of an evaluation: same buffers, the recorded graph again
        graph = graphed._graph
        with no_capture_fallback():
            before = calls["n"]
            graphed.reset(second).run(12, use_graph=True)
        assert graphed._graph is graph
        assert_graph_used(graphed)
        if inference:
            assert calls["n"] == before + 3                             # nothing is recorded again
        fresh = solver(second).run(12)
        _same_solvers(fresh, graphed, 12)
        assert first_difference(eager, fresh, ("z",)) is not None       # the second batch is another problem
    finally:
        if hook is not None:
            hook.remove()


# -------------------------------------------------------------------------------------------------------------- ADIL
def test_adil_learns_the_same_dictionary_file_with_and_without_graphs(tmp_path):
    """ADIL(method="gd") on resnet18, 2 epochs of 3 batches, the last one ragged, cached labels (the default).  The ragged
    batch is the third call, so the recording is made at ITS size: it is replayed in the second epoch with other rows, and
    the full batches take the eager fall-back.  The saved d, v, loss_all and fooling_rate_all are equal."""
    from attacks import ADIL
    e = engine()
    model = classifier("resnet18")
    n, k = 8 + 8 + 5, ATOMS
    images = byte_images(n, 64, 37)[1]
    g = torch.Generator().manual_seed(47)
    d0, v0 = -1 + 2 * torch.rand(3, 64, 64, k, generator=g), torch.rand(n, k, generator=g)
    epochs = [[p[:8], p[8:16], p[16:]] for p in (torch.randperm(n, generator=g).tolist() for _ in range(2))]
    learners = []

    class Recording(e.DictionaryLearner):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            learners.append(self)

    class Spy(ADIL):
        _learner_cls = Recording

    saved = {}
    for name, graph in (("eager", False), ("graphed", True)):
        with no_capture_fallback():
            Spy(model, eps=EPS_LEARNER, steps=2, n_atoms=k, batch_size=8, loss="logits", method="gd", init_d=d0, init_v=v0,
                data_train=_Items(images), data_val=None, model_name=name, dict_dir=str(tmp_path), epoch_batches=epochs,
                stream_dtype=BF16, use_graph=graph)
        saved[name] = torch.load(tmp_path / ("ImageNet_%s.bin" % name), map_location="cpu")
    a, b = saved["eager"], saved["graphed"]
    same_state({"d": a[0], "v": a[1]}, {"d": b[0], "v": b[1]}, ("d", "v"))
    assert a[2] == b[2] and a[3] == b[3] and len(a[2]) == len(a[3]) == 2
    assert len(learners) == 2 and learners[0]._graph is None
    assert_graph_used(learners[1])
    assert learners[1]._graph[5] == 5 and learners[1].sched_d.t == 6
    assert not torch.equal(a[0], d0)


# ------------------------------------------------------------------------------- the comparisons can fail: two shown
class _Scaled(torch.nn.Module):
    """A classifier whose logits are multiplied by a Python float: host state, read when a launch is issued."""

    def __init__(self, net, scale):
        super().__init__()
        self.net, self.scale = net, scale

    def forward(self, x):
        return self.net(x) * self.scale


def test_a_host_value_baked_into_the_recording_is_named_by_same_state():
    """The contract, documented by a failing comparison: a classifier's host state is read at capture.  Both learners see
    the same classifier object; its Python float changes after the capturing call.  The eager learner follows the change,
    the recording replays the launches it holds (the old factor), and same_state names `d`."""
    model = _Scaled(classifier("resnet18"), 1.0)
    n = 8
    images = byte_images(n, 64, 39)[1].to(DEV).to(BF16)
    a, b, _ = _learner_pair("resnet18", n, 49)
    index = torch.arange(n, device=DEV)
    _run_pair(model, a, b, [list(range(n))] * 4, lambda i: images, None)           # the third call records; one replay
    assert_graph_used(b)
    same_state(a, b, LEARNER_STATE)
    model.scale = -0.5                                                  # for both learners alike
    la, _ = a.step(model, images, index)
    lb, _ = b.step_graphed(model, images, index)
    assert float(la) != float(lb)
    diff = first_difference(a, b, LEARNER_STATE)
    assert diff is not None and diff.startswith("d differs in "), diff
    with pytest.raises(AssertionError, match=r"^d differs in \d+ of %d elements$" % a.d.numel()):
        same_state(a, b, LEARNER_STATE)


def test_a_failed_capture_falls_back_to_the_eager_loop_and_is_rejected(monkeypatch):
    """The fall-back branch of DDragueSolver.run: `_capture` is patched to raise (pure Python: nothing is captured).  The
    run warns, returns the eager loop's bits and leaves `_graph is False` — which `is not None` accepted and
    assert_graph_used rejects; inside no_capture_fallback() the same run is an error."""
    e = engine()
    model = classifier("resnet18")
    x = byte_images(8, 64, 35)[1].to(DEV).to(BF16)
    d = dictionary("resnet18", 5)
    eager = e.DDragueSolver(model, x, d, EPS_SOLVER, "logits").run(9)

    def refuse(self):
        raise RuntimeError("injected")

    monkeypatch.setattr(e.DDragueSolver, "_capture", refuse)
    with pytest.warns(RuntimeWarning, match="injected"):
        fell = e.DDragueSolver(model, x, d, EPS_SOLVER, "logits").run(9, use_graph=True)
    assert fell._graph is False and fell._graph is not None
    _same_solvers(eager, fell, 9)
    with pytest.raises(AssertionError, match="fell back to the eager loop"):
        assert_graph_used(fell)
    with pytest.raises(RuntimeWarning, match="injected"):
        with no_capture_fallback():
            e.DDragueSolver(model, x, d, EPS_SOLVER, "logits").run(9, use_graph=True)
    monkeypatch.undo()
    with no_capture_fallback():                                          # the unpatched solver does record
        real = e.DDragueSolver(model, x, d, EPS_SOLVER, "logits").run(9, use_graph=True)
    assert_graph_used(real)
    _same_solvers(eager, real, 9)


# ------------------------------------------------------------------- the collector stays out of the product's captures
class _Probe(torch.nn.Module):
    """Notes, at every forward that runs under capture, whether `ref` is dead and whether the collector is enabled."""

    def __init__(self, net, ref):
        super().__init__()
        self.net, self.ref, self.seen = net, ref, []

    def forward(self, x):
        if torch.cuda.is_current_stream_capturing():
            self.seen.append((self.ref() is None, gc.isenabled()))
        return self.net(x)


def test_a_dead_cycle_with_a_recorded_graph_is_collected_before_a_capture_not_inside_it():
    """What aborted a whole-suite run: the cyclic collector started in the middle of DDragueSolver._capture and destroyed a
    dead cycle that held an earlier recorded graph.  engine.capture_graph collects before the capture and holds the
    collector off during it.  Here a solver with a recorded graph is made garbage inside a cycle while the collector is
    off (so that nothing but capture_graph's own collection can free it, and no collection can fall into a capture
    whether the guard is there or not); at every classifier call of the next captures — the solver's and the learner's —
    it is already dead and the collector is disabled."""
    e = engine()
    model = classifier("resnet18")
    x = byte_images(8, 64, 35)[1].to(DEV).to(BF16)
    d = dictionary("resnet18", 5)
    index = torch.arange(8, device=DEV)
    was_enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        for use in ("solver", "learner"):
            with no_capture_fallback():
                old = e.DDragueSolver(model, x, d, EPS_SOLVER, "logits").run(6, use_graph=True)
            assert_graph_used(old)
            old.myself = old                                              # a cycle: only the collector frees it
            ref = weakref.ref(old)
            del old
            assert ref() is not None
            probe = _Probe(model, ref)
            with no_capture_fallback():
                if use == "solver":
                    new = e.DDragueSolver(probe, x, d, EPS_SOLVER, "logits").run(9, use_graph=True)
                else:
                    _, new, _ = _learner_pair("resnet18", 8, 49)
                    for _ in range(4):
                        new.step_graphed(probe, x, index)
            assert_graph_used(new)
            assert len(probe.seen) >= 2, probe.seen                       # forwards did run under capture
            assert all(dead and not enabled for dead, enabled in probe.seen), (use, probe.seen)
            assert not gc.isenabled()                                     # the state it found is the state it leaves
    finally:
        if was_enabled:
            gc.enable()
