"""ADIL attack class and Attack_dict_model on the MI355X kernels — drop-in for the reference's
attacks/attacks_classes/adil.py (constructor signature, attributes, dictionary file layout, return
conventions).  The per-batch PyTorch-op sequences of the reference are replaced by the fused HIP
solvers of dl_attack_on_imagenet_amd.engine; citations are to the reference's adil.py.

Deliberate fixes: the classifier is not differentiated w.r.t. its weights (Q8),
the dictionary file is read once per attack object, not once per call (Q7), the l1 projection never
syncs with the host (Q9), `alpha=` is accepted and ignored and output folders are created (Q14), and
the non-runnable code paths (Q15) raise a clear error or route to the working learner.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import engine, ops
from ..dist import DictGradReducer, global_epoch_batches, init_from_env, owned_rows, shard_bounds
from ..loader import ResidentImages, shuffled_batches
from .base import Attack
from .utils import QuickAttackDataset, clamp_image, constraint_dict, project_onto_l1_ball  # noqa: F401


class Attack_dict_model(nn.Module):
    """The learnable pair (d, v) with the synthesis x + D v[index] (adil.py:16-35)."""

    def __init__(self, d, v, eps):
        super().__init__()
        self.d = nn.Parameter(d)
        self.v = nn.Parameter(v)
        self.eps = eps

    def forward(self, x, index, model):
        # tensordot(v[index,:], d, ([1],[3])) + x as one fused kernel; differentiable in d and v (adil.py:24-27)
        return model(ops.dict_synth(x, self.d, self.v, index))

    def update_v(self):
        """Project every row of v onto the l1 ball of radius eps (adil.py:29-31)."""
        ops.l1ball_project_(self.v.data, float(self.eps))

    def update_d(self):
        """Clamp d to [-1, 1] (adil.py:33-35)."""
        self.d.data.clamp_(min=-1, max=1)


def engine_solve_codes(atk, images, d, mean_over=None, reducer=None):
    """forward_supervised_AdamW in 'train' mode on one rank's shard of a validation batch."""
    return engine.solve_codes_adamw(atk.model, images, d, atk.eps, atk.loss, atk.targeted, atk.kappa, atk.norm, 'train',
                                    mean_over=mean_over, reducer=reducer)


class ADIL(Attack):
    """ADiL — Adversarial Dictionary Learning (signature of adil.py:63-66).

    images (N,C,H,W) in [0,1], labels (N,) -> adversarial images (N,C,H,W) in [0,1] on `self.device`.
    Construction learns the dictionary if `trained_dicts/ImageNet_{model_name}.bin` is absent (adil.py:89-101).

    Extra keyword arguments (not in the reference, all optional):
      alpha          accepted and ignored (demo_dL_attack.py:114 passes it; the reference raises TypeError)
      init_d, init_v injected initial dictionary / raw codes instead of the device RNG draws of adil.py:145-150
      epoch_batches, val_batches   explicit batch order instead of the shuffled DataLoader (tests / multi-GPU parity)
      stream_dtype   torch.float32 (default) or torch.bfloat16 for the image-shaped streams x+Dv and dLoss/dx
      dict_dir       folder of the dictionary file (default 'trained_dicts')
      shuffle_seed   seed of the per-epoch global batches of the data-parallel learner (identical on every rank)
      cache_labels   learners: compute the clean pseudo-label of an image once (first epoch) instead of in every epoch
                     (engine.LabelCache; saves one of the two classifier forwards per step).  Default True since round 3:
                     the label of a frozen eval-mode classifier is a constant of the image, and 30 000 re-labellings in
                     shuffled / ragged batches changed none (profiles/r03_label_stability.md); False = the reference's op
                     sequence, which recomputes it every epoch (adil.py:172)
      val_every      validate (100 AdamW iterations per validation batch, adil.py:199-205) every this many epochs; the
                     reference does it after EVERY epoch but only prints the value and stores the last one, so any
                     setting writes the same dictionary file; 0 = after the last epoch only.  Default 1 (as upstream)
      upload_workers worker processes that fetch the dataset items for the one-time upload into HBM (loader.ResidentImages;
                     0 = in-process, right for in-memory tensors; > 0 for datasets that decode a JPEG per item)
      image_store    None (default): the learners keep the training / validation images resident in the stream dtype;
                     'uint8': as bytes, one per element (a quarter of the fp32 store, half of bf16 — ImageNet train
                     fits in 193 GB), for datasets of 8-bit images (u/255 values, ToTensor; a ValueError names the first
                     row that is not), and every learning step synthesizes straight from the bytes (ops.synth_store)
      use_graph      replay the learning step (engine.DictionaryLearner.step_graphed) and the DDrague inference iterations
                     (engine.DDragueSolver.run, three per launch) as hipGraph launches: for launch-bound uses — small
                     batches, the one-image attack of main.py; default: $ADIL_GRAPH == "1"
    """

    _learner_cls = engine.DictionaryLearner      # the fused (D, V) update; tests of the host logic may inject another

    def __init__(self, model, eps=None, steps=5e2, norm='linf', targeted=False, n_atoms=100, batch_size=100,
                 data_train=None, data_val=None, trials=10, attack='supervised', model_name=None, step_size=0.01,
                 is_distributed=False, steps_in=None, loss='ce', method='gd', warm_start=False, kappa=50,
                 steps_inference=30, alpha=None, init_d=None, init_v=None, epoch_batches=None, val_batches=None,
                 stream_dtype=None, dict_dir='trained_dicts', shuffle_seed=0, use_graph=None, cache_labels=True, val_every=1,
                 upload_workers=0, image_store=None):
        if image_store not in (None, 'uint8'):
            raise ValueError(f"image_store must be None or 'uint8', got {image_store!r}")
        super().__init__("ADIL", model.eval())
        self.norm = norm.lower()
        self.eps = eps
        self.n_atoms = n_atoms
        self.dictionary = None
        self.targeted = targeted
        self.attack = attack
        self.trials = trials
        self.step_size = step_size
        self.steps_inference = steps_inference
        self.steps = steps
        self.steps_inner = steps_in
        self.batch_size = batch_size
        self.loss = loss
        self.model_name = model_name
        self.method = method
        self.kappa = kappa
        self.stream_dtype = stream_dtype
        self._init_d, self._init_v = init_d, init_v
        self._epoch_batches, self._val_batches = epoch_batches, val_batches
        self._shuffle_seed = int(shuffle_seed)
        self._use_graph = (os.environ.get("ADIL_GRAPH") == "1") if use_graph is None else bool(use_graph)
        self._cache_labels = bool(cache_labels)
        self._val_every = int(val_every)
        self._upload_workers = int(upload_workers)
        self.image_store = image_store
        self._pinv = None
        self._solvers = {}
        self._dict_mtime = None
        self.model_file = os.path.join(dict_dir, f"ImageNet_{model_name}.bin")

        if not os.path.exists(self.model_file):
            if data_train is None:
                return                           # nothing to learn from yet; forward() reports it
            if is_distributed:
                self.learn_dictionary_distributed(data_train, data_val)
            elif method == 'gd':
                self.learn_dictionary_a(dataset=data_train, val=data_val, warm_start=warm_start)
            elif method == 'alter':
                self.learn_dictionary_b(dataset=data_train, val=data_val, warm_start=warm_start)
            else:
                raise ValueError(f"unknown method {method!r} (expected 'gd' or 'alter')")

    # ------------------------------------------------------------------ helpers
    _MAX_SOLVERS = 4          # graphed DDrague solvers kept per batch shape (e.g. the full batch + a ragged last one)

    def f_loss(self, outputs, labels):
        """CW-style margin (adil.py:103-112); `self._targeted` (always False) selects the branch, as upstream."""
        return engine.margin_loss(outputs, labels, self.kappa, self._targeted)

    def _cast(self, x):
        x = x.to(device=self.device)
        if self.stream_dtype is not None:
            x = x.to(self.stream_dtype)
        return x.contiguous()

    def _dataset_shape(self, dataset):
        dataset.indexed = False
        x, _ = dataset[0]
        return len(dataset), tuple(x.shape)

    def _initial_dictionary(self, shape, warm_start):
        nc, nx, ny = shape
        if self._init_d is not None:
            return self._init_d.to(device=self.device, dtype=torch.float32).contiguous().clone()
        if warm_start:                                                       # adil.py:139-143
            path = os.path.join("dict_model_ImageNet_version_constrained",
                                f"ImageNet_{self.model_name}_num_atom_{self.n_atoms}_nepoch_{self.steps}_AdamW_200.bin")
            d = torch.load(path, map_location="cpu")[0]
            return d.to(device=self.device, dtype=torch.float32).contiguous()
        if self.norm == 'l2':                                                # adil.py:145-146
            return self.projection_d(torch.randn(nc, nx, ny, self.n_atoms, device=self.device))
        return -1 + 2 * torch.rand(nc, nx, ny, self.n_atoms, device=self.device)   # adil.py:148

    def _resident(self, dataset, rows=None):
        """The data step in front of the path: the dataset (or this rank's rows of it) resident in HBM in the stream
        dtype, or as bytes (image_store='uint8'); replaces the per-item DataLoader of adil.py:130-133 (see loader.py)."""
        if self.image_store == 'uint8':
            return ResidentImages(dataset, self.device, torch.uint8, rows=rows, num_workers=self._upload_workers,
                                  stream_dtype=self.stream_dtype or torch.float32)
        return ResidentImages(dataset, self.device, self.stream_dtype or torch.float32, rows=rows,
                              num_workers=self._upload_workers)

    @staticmethod
    def _epoch_order(n, batch_size, explicit, epoch):
        """Index batches of one epoch: injected (tests / multi-GPU parity) or the reference's shuffled DataLoader order."""
        if explicit is not None:
            return [[int(i) for i in idx] for idx in explicit[epoch]]
        return shuffled_batches(n, batch_size)

    def _labelled_batches(self, train, order):
        """(index, x, labels) per batch; labels is None (the learner recomputes them, adil.py:172) unless cache_labels.
        For an 8-bit store x is the store itself (the learner synthesizes from its rows `index`); a clean batch is
        gathered only for a label that is not cached yet."""
        order = [list(idx) for idx in order]
        if self._cache_labels and getattr(train, "_label_cache", None) is None:
            train._label_cache = engine.LabelCache(len(train), self.device)
        if getattr(train, "is_bytes", False):
            for rows in order:
                index = train.index_tensor(rows)
                yield index, train, (train._label_cache.get(self.model, lambda index=index: train.gather(index), index, rows)
                                     if self._cache_labels and len(rows) else None)
            return
        for rows, (index, x) in zip(order, train.batches(order)):
            yield index, x, (train._label_cache.get(self.model, x, index, rows) if self._cache_labels and len(rows) else None)

    def _val_due(self, iteration):
        return self._val_every > 0 and (iteration + 1) % self._val_every == 0

    def _skip_validation(self, val, batch_size):
        """An epoch whose validation is skipped (val_every) still draws what the validation loader's iterator would have
        drawn from the global torch RNG (its base seed + the sampler's seed, loader.shuffled_batches), so the training
        shuffle of every later epoch — and with it the dictionary file — is the same for any val_every."""
        self._rng_before_skip = None
        if val is not None and self._val_batches is None:
            self._rng_before_skip = torch.get_rng_state()        # the end-of-run validation replays exactly these draws
            shuffled_batches(len(val), batch_size)

    def _final_validation(self, val, epoch, d, batch_size):
        """The stored validation value is the last epoch's (adil.py:199-205, :210); when that epoch's validation was
        skipped it runs here, with the shuffle the skipped call would have used."""
        state = getattr(self, "_rng_before_skip", None)
        if state is not None:
            torch.set_rng_state(state)
        return self._validate(val, epoch, d, batch_size)

    def _validate(self, val, epoch, d, batch_size):
        """Per-epoch validation through forward_supervised_AdamW in 'train' mode (adil.py:199-205).
        `val` is a ResidentImages (or None)."""
        if val is None:
            return torch.zeros((), device=self.device)
        fooled = torch.zeros((), dtype=torch.int64, device=self.device)
        for _, x in val.batches(self._epoch_order(len(val), batch_size, self._val_batches, epoch)):
            fooled += self.forward_supervised_AdamW(x, None, d, 'train')
        return fooled / len(val)

    def _save(self, d, v, loss_all, fooling_rate_all, val_fool):
        """[D (C,H,W,K), V (N,K), loss_all, fooling_rate_all, val_fool] — the reference's on-disk layout
        (adil.py:210,332); the loader only uses element 0 (adil.py:444-445)."""
        folder = os.path.dirname(self.model_file)
        if folder:
            os.makedirs(folder, exist_ok=True)
        torch.save([d, v, loss_all, fooling_rate_all, val_fool], self.model_file)

    # ------------------------------------------------------------------ learners
    def learn_dictionary_a(self, dataset, val, warm_start):
        """Joint AdamW learning of (D, V) — learn_dictionary_a (adil.py:114-210)."""
        n_img, shape = self._dataset_shape(dataset)
        batch_size = n_img if self.batch_size is None else self.batch_size
        train = self._resident(dataset)
        val_res = self._resident(val) if val is not None else None

        d = self._initial_dictionary(shape, warm_start)
        v0 = self._init_v if self._init_v is not None else torch.rand(n_img, self.n_atoms, device=self.device)
        v = self.projection_v(v0.to(device=self.device, dtype=torch.float32))               # adil.py:150
        learner = self._learner_cls(d, v, self.eps, self.step_size, self.loss, self.targeted, self.kappa)

        loss_all, fooling_rate_all = [], []
        val_fool = torch.zeros((), device=self.device)
        validated = True
        for iteration in range(int(self.steps)):
            loss_full = torch.zeros((), dtype=torch.float32, device=self.device)
            fooled = torch.zeros((), dtype=torch.int64, device=self.device)
            for index, x, lab in self._labelled_batches(train, self._epoch_order(n_img, batch_size, self._epoch_batches, iteration)):
                if self._use_graph:
                    ls, fl = learner.step_graphed(self.model, x, index, lab)
                else:
                    ls, fl = learner.step(self.model, x, index, lab)                       # adil.py:168-191
                loss_full += ls
                fooled += fl
            loss_all.append(loss_full.item() / n_img)                                      # adil.py:194
            fooling_rate_all.append(fooled.item() / n_img)                                 # adil.py:195
            print(loss_all[-1], fooling_rate_all[-1])
            validated = self._val_due(iteration)
            if validated:
                val_fool = self._validate(val_res, iteration, learner.d, batch_size)
                print(float(val_fool))
            else:
                self._skip_validation(val_res, batch_size)
            if iteration > 1 and abs(loss_all[iteration] - loss_all[iteration - 1]) < 1e-6:    # adil.py:207
                break
        if loss_all and not validated:                                   # the stored value is the last epoch's
            val_fool = self._final_validation(val_res, len(loss_all) - 1, learner.d, batch_size)
        self._save(learner.d, learner.v, loss_all, fooling_rate_all, val_fool)
        return learner

    def learn_dictionary_b(self, dataset, val, warm_start):
        """Alternating scheme — learn_dictionary_b (adil.py:212-332): `steps_inner` epochs of V-steps (AdamW lr
        step_size) then `steps_inner` epochs of D-steps (AdamW lr 2*step_size)."""
        n_img, shape = self._dataset_shape(dataset)
        batch_size = n_img if self.batch_size is None else self.batch_size
        train = self._resident(dataset)
        val_res = self._resident(val) if val is not None else None

        d = self._initial_dictionary(shape, warm_start)
        v0 = self._init_v if self._init_v is not None else torch.zeros(n_img, self.n_atoms, device=self.device)
        v = self.projection_v(v0.to(device=self.device, dtype=torch.float32))               # adil.py:246
        learner = self._learner_cls(d, v, self.eps, self.step_size, self.loss, self.targeted, self.kappa,
                                    lr_d=2 * self.step_size, lr_v=self.step_size)           # adil.py:250-251
        loss_all, fooling_rate_all = [], []
        val_fool = torch.zeros((), device=self.device)
        validated = True
        epoch = 0
        for iteration in range(int(self.steps // self.steps_inner)):
            for _ in range(self.steps_inner):                                              # V-steps, adil.py:265-289
                for index, x, lab in self._labelled_batches(train, self._epoch_order(n_img, batch_size, self._epoch_batches, epoch)):
                    learner.step_codes(self.model, x, index, lab)
                epoch += 1
            for _ in range(self.steps_inner):                                              # D-steps, adil.py:292-314
                fooled = torch.zeros((), dtype=torch.int64, device=self.device)
                ls = None
                for index, x, lab in self._labelled_batches(train, self._epoch_order(n_img, batch_size, self._epoch_batches, epoch)):
                    ls, fl = learner.step_dictionary(self.model, x, index, lab)
                    fooled += fl
                epoch += 1
            loss_all.append(ls.item() / n_img)               # last batch only — reference quirk Q11 (adil.py:313-317)
            fooling_rate_all.append(fooled.item() / n_img)
            print('d_step: ', loss_all[-1], fooling_rate_all[-1])
            validated = self._val_due(iteration)
            if validated:
                val_fool = self._validate(val_res, iteration, learner.d, batch_size)
            else:
                self._skip_validation(val_res, batch_size)
            if iteration > 1 and abs(loss_all[iteration] - loss_all[iteration - 1]) < 1e-6:    # adil.py:329
                break
        if loss_all and not validated:
            val_fool = self._final_validation(val_res, len(loss_all) - 1, learner.d, batch_size)
        self._save(learner.d, learner.v, loss_all, fooling_rate_all, val_fool)
        return learner

    def learn_dictionary_distributed(self, dataset, val=None):
        """Data-parallel learn_dictionary_a: one process per GPU (torchrun env).  Rank r OWNS a contiguous shard of the
        images, keeps them resident in its HBM together with their code rows and AdamW moments; D is replicated.
        Every step is one GLOBAL batch: each rank processes the members it owns, ONE all-reduce(SUM) of grad_d makes
        the dictionary gradient the global batch's, and the identical fused AdamW keeps D bit-identical across ranks.
        The global batches come from `epoch_batches` when injected, otherwise from dist.global_epoch_batches (seeded,
        identical on all ranks, balanced); either way every rank takes the same number of steps — a rank that owns
        nothing of a batch contributes a zero gradient — so collectives always pair up (ragged shards included).
        Validation (adil.py:199-205) is sharded the same way and its fooled counts are summed.
        Replaces adil.py:334-430, which deadlocks as written (the loop sits under `if rank == 0`); the parity target
        is the single-process learner at the global batch."""
        rank, world, local_rank = init_from_env()
        if not torch.distributed.is_initialized():
            return self.learn_dictionary_a(dataset, val, False)
        reducer = DictGradReducer()
        n_img, shape = self._dataset_shape(dataset)
        batch_size = n_img if self.batch_size is None else self.batch_size
        lo, hi = shard_bounds(n_img, rank, world)
        train = self._resident(dataset, rows=range(lo, hi))
        val_res, vlo, vhi = None, 0, 0
        if val is not None:
            vlo, vhi = shard_bounds(len(val), rank, world)
            val_res = self._resident(val, rows=range(vlo, vhi))

        d = self._initial_dictionary(shape, False)
        reducer.broadcast_(d, 0)                                                  # identical D0 on every rank
        v0 = self._init_v[lo:hi] if self._init_v is not None else torch.rand(hi - lo, self.n_atoms, device=self.device)
        v = self.projection_v(v0.to(device=self.device, dtype=torch.float32))
        learner = self._learner_cls(d, v, self.eps, self.step_size, self.loss, self.targeted, self.kappa,
                                    reducer=reducer)
        def validate(epoch):
            """Sharded validation (adil.py:199-205): every rank solves the codes of the images it owns, counts are summed."""
            if self._val_batches is not None:
                vorder = self._val_batches[epoch]
            else:
                vorder = global_epoch_batches(len(val), batch_size, world, self._shuffle_seed + 1, epoch)
            vfooled = torch.zeros((), dtype=torch.int64, device=self.device)
            for gb in vorder:
                mine = [i - vlo for i in owned_rows(gb, vlo, vhi)]
                vfooled += engine_solve_codes(self, val_res.gather(mine), learner.d, mean_over=len(gb), reducer=reducer)
            return torch.tensor(reducer.sum_scalars(vfooled)[0] / len(val), device=self.device)

        loss_all, fooling_rate_all = [], []
        val_fool = torch.zeros((), device=self.device)
        validated = True
        for iteration in range(int(self.steps)):
            loss_full = torch.zeros((), dtype=torch.float32, device=self.device)
            fooled = torch.zeros((), dtype=torch.int64, device=self.device)
            if self._epoch_batches is not None:
                order = self._epoch_batches[iteration]
            else:
                order = global_epoch_batches(n_img, batch_size, world, self._shuffle_seed, iteration)
            local = [[i - lo for i in owned_rows(gb, lo, hi)] for gb in order]
            for index, x, lab in self._labelled_batches(train, local):
                ls, fl = learner.step(self.model, x, index, lab)
                loss_full += ls
                fooled += fl
            tot_loss, tot_fooled = reducer.sum_scalars(loss_full, fooled)         # adil.py:418-419
            loss_all.append(tot_loss / n_img)
            fooling_rate_all.append(tot_fooled / n_img)
            if rank == 0:
                print(loss_all[-1], fooling_rate_all[-1])
            validated = self._val_due(iteration)
            if val_res is not None and validated:
                val_fool = validate(iteration)
            if iteration > 1 and abs(loss_all[iteration] - loss_all[iteration - 1]) < 1e-6:
                break
        if val_res is not None and loss_all and not validated:
            val_fool = validate(len(loss_all) - 1)
        counts = [shard_bounds(n_img, r, world)[1] - shard_bounds(n_img, r, world)[0] for r in range(world)]
        v_all = reducer.gather_rows(learner.v, counts)                           # once, at the end (not in the data path)
        if rank == 0:
            self._save(learner.d, v_all, loss_all, fooling_rate_all, val_fool)
        torch.distributed.barrier()
        return learner

    # ------------------------------------------------------------------ inference
    def _load_dictionary(self):
        mtime = os.path.getmtime(self.model_file)
        if self.dictionary is None or self._dict_mtime != mtime:
            rlts = torch.load(self.model_file, map_location="cpu")
            self.dictionary = rlts[0].to(device=self.device, dtype=torch.float32).contiguous()   # adil.py:444-445
            self._dict_mtime = mtime
            self._pinv = None
        return self.dictionary

    def forward(self, images, labels):
        """attack(images, labels) (adil.py:432-458)."""
        images = images.to(self.device)
        labels = labels.to(self.device)
        if not os.path.exists(self.model_file):
            raise FileNotFoundError(
                f"The adversarial dictionary {self.model_file} has not been learned: construct ADIL with "
                "data_train=... first (the reference's fallback calls a method that does not exist, adil.py:442)")
        d = self._load_dictionary()
        if images.shape[0] == 0:                             # e.g. performance() kept no correctly classified sample
            return images.clone() if self.attack == 'supervised' else (images.clone(), [])
        if self.attack == 'supervised':
            return self.forward_supervised_DDrague(images, labels, d)
        return self.forward_unsupervised(images)

    def forward_unsupervised(self, images):
        """Sample `trials` code matrices and keep the best adversarial image per sample (adil.py:460-506).
        Returns (adv_images_best, dv_norm_inf) like the reference."""
        if self.dictionary is None:
            self._load_dictionary()
        images = self._cast(images)
        samples = [self.sample_sphere(images.shape[0]) for _ in range(int(self.trials))]
        adv, dv_norm = engine.attack_unsupervised(self.model, images, self.dictionary, self.eps, samples)
        return adv, dv_norm.tolist()

    def forward_supervised_DDrague(self, images, labels, d):
        """Optimise z with the perturbation D D_dagger z (adil.py:508-567); the default inference.  With use_graph the
        iterations are replayed from a hipGraph (three per launch) and the solver — buffers and graph — is kept per
        batch shape, so every batch of an evaluation after the first reuses the recorded graph."""
        if self._pinv is None or self._pinv.d is not d:
            self._pinv = engine.PseudoInverse(d)
            self._solvers = {}
        images = self._cast(images)
        if not self._use_graph:
            return engine.solve_ddrague(self.model, images, d, self.eps, self.steps_inference, self.loss,
                                        self.targeted, self.kappa, pinv=self._pinv)
        key = (tuple(images.shape), images.dtype)
        solver = self._solvers.pop(key, None)
        if solver is None:
            while len(self._solvers) >= self._MAX_SOLVERS:        # a solver holds z, m, s and its graph: keep a few shapes
                self._solvers.pop(next(iter(self._solvers)))      # (oldest first; dicts keep insertion order)
            solver = engine.DDragueSolver(self.model, images, d, self.eps, self.loss, self.targeted, self.kappa,
                                          pinv=self._pinv)
        else:
            solver.reset(images)
        self._solvers[key] = solver                                # most recently used last
        return solver.run(self.steps_inference, use_graph=True).result()[0]

    def forward_supervised_AdamW(self, images, labels, d, model='train'):
        """Optimise the codes with D fixed (adil.py:569-623). 'train' -> fooled count, else adversarial images."""
        return engine.solve_codes_adamw(self.model, self._cast(images), d, self.eps, self.loss, self.targeted,
                                        self.kappa, self.norm, model)

    # ------------------------------------------------------------------ projections / sampling
    def projection_v(self, var):
        """adil.py:625-633: l2 -> eps * v / max(||v||, eps); linf -> l1 ball of radius eps."""
        out = var.detach().to(device=self.device, dtype=torch.float32).contiguous().clone()
        if self.norm == 'l2':
            return ops.l2ball_project_(out, float(self.eps))
        if self.norm == 'linf':
            return ops.l1ball_project_(out, float(self.eps))
        raise ValueError(f"unknown norm {self.norm!r}")

    def projection_d(self, var):
        """adil.py:635-642: l2 -> per-atom unit l2 ball; linf -> clamp to [-1, 1]."""
        if self.norm == 'l2':
            return constraint_dict(var.contiguous(), constr_set='l2ball')
        if self.norm == 'linf':
            return torch.clamp(var, min=-1, max=1)
        raise ValueError(f"unknown norm {self.norm!r}")

    def sample_sphere(self, n_samples):
        """adil.py:644-655 (draws from the CPU torch RNG like the reference, then moves to the device)."""
        if self.norm == 'l2':
            var = 2 * torch.rand(n_samples, self.n_atoms) - 1
            return (self.eps * var / var.norm(p='fro', dim=1, keepdim=True)).to(self.device)
        if self.norm == 'linf':
            u = torch.rand(n_samples, self.n_atoms, 1)[:, :, 0]
            return self.projection_v(self.eps + (2 * self.eps - self.eps) * u)
        raise ValueError(f"unknown norm {self.norm!r}")
