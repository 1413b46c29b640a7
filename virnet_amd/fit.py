"""The training loops on the device.  Denoising: what train_denoising_syn.py:153-273 and train_denoising_real.py:147-262 do per process, from
the pieces of this package, with the host reading the device once per print interval instead of six times per step.

    pool = datagen.ImagePool(uint8_images, "cuda")
    out = fit_denoising(net, pool, cfg, val=datagen.SimulateTestSet(test_pool), save_dir="train_record")

Per step: :mod:`datagen` builds the batch, ``net(x)`` records the fused step, :func:`elbo.elbo_denoising` gives the loss and its
gradients, :class:`optim.ClipAdam` clips and steps, and :class:`trainlog.StepLog` takes the six scalars the reference reads with
``.item()`` (:187-198).  None of these synchronises; the loop reads the log at the first step, at every ``print_freq``-th step and at the
end of the epoch, where it prints the reference's lines.  The learning rates are :func:`schedule.warmup_cosine`'s list, indexed by the
epoch.  One process takes the module as it is given (a wrapper such as ``dist.DistributedTrainer`` keeps its own).

Across ranks (``torch.distributed`` initialised, world above one -- ``dist.init()`` under torchrun, or a driver's ``--gpus N``) the same call
is one rank of a data-parallel job.  ``cfg["batch_size"]`` is the GLOBAL batch and must divide by the world size.  Every rank draws the whole
batch's parameters from the same ``random.Random`` (host-only, cheap, and it keeps all ranks and all world sizes in lockstep) and synthesises
only its rows ``dist.shard_range(batch, world, rank)`` under their global sample ids: ``datagen`` is keyed by sample id, so the ranks' batches
concatenated are bit for bit the one-process batch.  A real-noise row brings its MixUp partner along (:func:`shard_real_params`).  Rank 0's
parameters are broadcast once (not on ``resume``: every rank loads the file), one ``dist.GradientReducer`` averages the gradients exactly
once per step -- fed from inside the fused backward, or by ``reduce_grads()`` after a per-conv backward -- and ``ClipAdam`` clips the
AVERAGED gradients, so ``grad_norms`` agree on all ranks.  Every rank keeps its ``StepLog`` (its own shard's loss terms); only rank 0 calls
``log``, runs the test stage and writes checkpoints; at the end of every epoch the ranks compare one fp64 checksum of their parameters.
Not done here: the validation set is not sharded, and the per-conv backward does not feed the reducer layer by layer.

Randomness, per epoch ``e`` (the reference's ``reset_seed(e)``): the crops, sigma maps and augmentation flags come from
``random.Random(e)`` in the reference's order; the synthetic noise is drawn on the device with ``seed=e`` and sample ids ``step *
batch_size + i``; the real-noise loop also seeds torch's global CPU generator with ``e`` for the MixUp draws (``RealTrain.reset_seed``
leaves that generator alone, so the reference's own MixUp stream is not reproducible across a resume; here it is).  A run that is
stopped after an epoch and resumed from its checkpoint therefore continues bit for bit.

:func:`fit_sisr` is the same for train_SISR.py:185-333: ``datagen.sisr_batch``, ``net(im_lr, sf)``, :func:`elbo.elbo_sisr`, three clip sets,
eight logged scalars, :func:`schedule.cosine`, ``random.Random(e * 1000)`` and ``torch.manual_seed(e * 1000)`` per epoch, and a test stage per
noise type on a :class:`datagen.GeneralTestSet` with the training scripts' float-Y metric (``metrics.psnr_ssim(..., ycbcr="float")``).

Weight average: the optional config keys ``ema_decay`` / ``ema_warmup`` switch on an exponential moving average of the parameters
(:class:`ema.WeightEMA`: shadow tensors updated by one launch per 64 tensors after every step, no host sync); the test stage then runs
on the averaged weights, swapped in and out in place, and the checkpoint carries them as ``ema_state_dict``.  Off by default, and then
nothing differs.

Summaries: with ``writer=`` (a ``preview.FolderWriter``, a tensorboard ``SummaryWriter``) the loops write what the reference writes -- the loss
at every printed step, the epoch's loss and test scalars, and the image grids of its previews, formed on the device (:mod:`preview`) from
tensors the step already has at steps where the log is read anyway, one host copy per event; ``step_img`` counts the events.  Off by
default, and then nothing is launched, allocated or imported; with a writer the run itself is the same bit for bit.

There is ONE loop, :func:`_fit`: resume, the epochs and their steps, the log reads and lines, the checkpoints and the returned dictionary.
What the two tasks do differently reaches it as a :class:`_Task`, a record that ``fit_denoising`` and ``fit_sisr`` fill in after reading
their config and running their own argument checks.  Likewise one config reader (:func:`_read`, with a schema per task), one validation
body (:func:`_validate`) and one optimizer constructor (:func:`_optimizer`) serve both.
"""
from __future__ import annotations

import os
import random
import time
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import datagen, elbo, metrics
from .optim import ClipAdam
from .schedule import cosine, warmup_cosine
from .trainlog import StepLog

LOG_NAMES = ("Loss", "lh", "KLG", "KLIG", "GNorm_R", "GNorm_S")
SISR_LOG_NAMES = ("Loss", "lh", "KLR", "KLS", "KLK", "GNorm_R", "GNorm_S", "GNorm_K")
NOISE_TYPES = ("Gaussian", "JPEG")
DEFAULTS = {"lr_min": 1e-6, "print_freq": 100, "steps_per_epoch": 10000}          # (the reference's dataset length is 10000 * batch_size)
VAL_BATCH = 8          # images per validation forward (a same-shape group is cut into chunks of this many)
# the previews of a run with a summary writer: a train event every so many print intervals (train_denoising_syn.py:201, train_SISR.py:246),
# a test event every so many validation images (train_denoising_syn.py:238, train_SISR.py:290)
PREVIEW_EVERY, SISR_PREVIEW_EVERY = 50, 20
TEST_PREVIEW_EVERY, SISR_TEST_PREVIEW_EVERY = 20, 3


# ---- configs ---------------------------------------------------------------------------------------------------------------------------------
# a reader's schema: the keys that must be there; the integer keys, each with the smallest value allowed (1, or 0 for a count that may be
# zero); the non-negative floats; the booleans; the pairs of numbers.  DEFAULTS' keys are read whether required or not.
SCHEMA = dict(
    required=("batch_size", "patch_size", "epochs", "warmup_epochs", "lr", "clip_grad_R", "clip_grad_S", "var_window", "eps2"),
    ints={"batch_size": 1, "patch_size": 1, "epochs": 1, "warmup_epochs": 0, "print_freq": 1, "steps_per_epoch": 1, "var_window": 1},
    floats=("lr", "lr_min", "clip_grad_R", "clip_grad_S", "eps2"))
SISR_SCHEMA = dict(
    required=("batch_size", "hr_size", "epochs", "lr", "sf", "k_size", "downsampler", "add_jpeg", "kernel_shift", "noise_level", "noise_jpeg",
              "eps2", "r2", "var_window", "kappa0", "penalty_K", "clip_grad_R", "clip_grad_S", "clip_grad_K"),
    ints={"batch_size": 1, "hr_size": 1, "epochs": 1, "print_freq": 1, "steps_per_epoch": 1, "var_window": 1, "sf": 1, "k_size": 1},
    floats=("lr", "lr_min", "clip_grad_R", "clip_grad_S", "clip_grad_K", "eps2", "r2", "kappa0"),
    bools=("add_jpeg", "kernel_shift"), pairs=("noise_level", "noise_jpeg", "penalty_K"))


def str2bool(v, key: str = "flag") -> bool:
    """``util_opts.str2bool``: the reference's configs spell booleans as the strings "True" / "False" (any case); a Python bool passes."""
    if isinstance(v, bool):
        return v
    if isinstance(v, str) and v.lower() in ("true", "false"):
        return v.lower() == "true"
    raise ValueError(f"cfg[{key!r}] = {v!r}: the string 'True' or 'False' is expected")


def _read(cfg: dict, required, ints, floats, bools=(), pairs=()) -> dict:
    """A schema's keys out of ``cfg``, each checked and converted to its type.  Checks between keys are the caller's."""
    if not isinstance(cfg, dict):
        raise TypeError(f"cfg must be a dict of the reference's config keys, got {type(cfg).__name__}")
    missing = [k for k in required if k not in cfg]
    if missing:
        raise KeyError(f"cfg lacks {missing}")
    c = {k: cfg.get(k, DEFAULTS.get(k)) for k in required + tuple(DEFAULTS)}
    for k, least in ints.items():
        v = c[k]
        if isinstance(v, (bool, str)) or int(v) != v or int(v) < least:
            raise ValueError(f"cfg[{k!r}] = {v!r}: a {'positive' if least else 'non-negative'} integer is expected")
        c[k] = int(v)
    for k in floats:
        v = c[k]
        if isinstance(v, (bool, Tensor)) or not isinstance(v, (int, float)) or not float(v) >= 0.0:
            raise ValueError(f"cfg[{k!r}] = {v!r}: a non-negative float is expected")
        c[k] = float(v)
    for k in bools:
        c[k] = str2bool(c[k], k)
    for k in pairs:
        v = c[k]
        if not isinstance(v, (list, tuple)) or len(v) != 2 or any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in v):
            raise ValueError(f"cfg[{k!r}] = {v!r}: a list of two numbers is expected")
        c[k] = [float(v[0]), float(v[1])]
    return c


def _read_ema(cfg: dict) -> dict:
    """The two optional keys of the weight average (ema.py): ``ema_decay`` -- absent, None or 0: off (None here), else a float in (0, 1) --
    and ``ema_warmup``, a bool or the string "True" / "False"."""
    decay, warmup = cfg.get("ema_decay"), str2bool(cfg.get("ema_warmup", False), "ema_warmup")
    if decay is not None:
        if isinstance(decay, (bool, str, Tensor)) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"cfg['ema_decay'] = {decay!r}: a float with 0 <= ema_decay < 1 is expected (0 or None: no weight average)")
        decay = float(decay) or None
    return {"ema_decay": decay, "ema_warmup": warmup}


def read_config(cfg: dict) -> dict:
    """The loop's settings out of a reference config (configs/denoising_syn.json, configs/denoising_real.json; other keys are ignored),
    checked: ints for the counts, positive floats for the rates; plus the optional ``ema_decay`` / ``ema_warmup`` (:func:`_read_ema`)."""
    c = _read(cfg, **SCHEMA)
    c.update(_read_ema(cfg))
    if c["epochs"] <= c["warmup_epochs"]:
        raise ValueError(f"cfg: epochs {c['epochs']} must exceed warmup_epochs {c['warmup_epochs']}")
    return c


def read_sisr_config(cfg: dict) -> dict:
    """The SISR loop's settings out of a reference config (configs/sisr_x2.json, sisr_x3.json, sisr_x4.json; other keys are ignored),
    checked: ints for the counts, non-negative floats for the rates, the booleans from their strings, ``noise_level`` / ``noise_jpeg``
    as increasing pairs and ``penalty_K`` as a pair; plus the optional ``ema_decay`` / ``ema_warmup`` (:func:`_read_ema`)."""
    c = _read(cfg, **SISR_SCHEMA)
    c.update(_read_ema(cfg))
    for k in ("noise_level", "noise_jpeg"):
        if not c[k][0] < c[k][1]:
            raise ValueError(f"cfg[{k!r}] = {c[k]!r}: an increasing pair is expected")
    if not isinstance(c["downsampler"], str) or c["downsampler"].lower() not in ("direct", "bicubic"):
        raise ValueError(f"cfg['downsampler'] = {c['downsampler']!r}: 'Direct' or 'Bicubic' is expected")
    if c["hr_size"] % c["sf"]:
        raise ValueError(f"cfg: hr_size {c['hr_size']} is not a multiple of sf {c['sf']}")
    if c["kappa0"] <= 1.0:
        raise ValueError(f"cfg['kappa0'] = {c['kappa0']!r}: the Gamma draw has concentration kappa0 - 1 and needs kappa0 > 1")
    return c


def strip_json_comments(text: str) -> str:
    """JSON with ``#`` comments (the reference's config files, which it reads with commentjson) -> plain JSON: a ``#`` outside a string
    starts a comment that runs to the end of its line; inside a string (escapes respected) it is an ordinary character."""
    out, in_string, escaped, i = [], False, False, 0
    while i < len(text):
        ch = text[i]
        if in_string:
            out.append(ch)
            if escaped:
                escaped = False
            elif ch == "\\":
                escaped = True
            elif ch == '"':
                in_string = False
        elif ch == '"':
            in_string = True
            out.append(ch)
        elif ch == "#":
            while i < len(text) and text[i] not in "\r\n":
                i += 1
            continue
        else:
            out.append(ch)
        i += 1
    return "".join(out)


def load_config(path) -> dict:
    """A reference config file as a dict (JSON with ``#`` comments; a trailing comma before ``}`` or ``]`` is not accepted, as in JSON)."""
    import json
    with open(os.fspath(path), "r") as f:
        return json.loads(strip_json_comments(f.read()))


# ---- clip sets and the optimizer ---------------------------------------------------------------------------------------------------------------
def _clip_sets(net: torch.nn.Module, keys: Sequence[str]) -> Tuple[List[Tensor], ...]:
    named = list(net.named_parameters())
    return tuple([p for n, p in named if key in n.lower()] for key in keys)


def _optimizer(net: torch.nn.Module, c: dict, keys: Sequence[str]) -> ClipAdam:
    """Adam with one clip set per key: ``rnet`` is clipped at ``clip_grad_R``, ``snet`` at ``clip_grad_S``, ``knet`` at ``clip_grad_K``."""
    return ClipAdam(net.parameters(), lr=c["lr"], clip=[(ps, c["clip_grad_" + key[0].upper()]) for key, ps in zip(keys, _clip_sets(net, keys))])


def clip_sets(net: torch.nn.Module) -> Tuple[List[Tensor], List[Tensor]]:
    """(param_R, param_S) of train_denoising_syn.py:153-154: the parameters whose lower-cased name contains ``rnet`` / ``snet``."""
    return _clip_sets(net, ("rnet", "snet"))


def sisr_clip_sets(net: torch.nn.Module) -> Tuple[List[Tensor], List[Tensor], List[Tensor]]:
    """(param_rnet, param_snet, param_knet) of train_SISR.py:182-184: the parameters whose lower-cased name contains the key."""
    return _clip_sets(net, ("rnet", "snet", "knet"))


def sisr_optimizer(net: torch.nn.Module, c: dict) -> ClipAdam:
    """Adam with the three clip sets of train_SISR.py:98,182-184,226-228."""
    return _optimizer(net, c, ("rnet", "snet", "knet"))


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------------
def checkpoint_dict(net: torch.nn.Module, opt: Optional[torch.optim.Optimizer], epoch: int, step: int, step_img: Dict[str, int],
                    phases: Sequence[str] = ("train", "test"), ema=None) -> dict:
    """The reference's checkpoint (train_denoising_syn.py:262-268) -- ``epoch`` (epochs finished), ``step``, ``step_img``,
    ``model_state_dict`` -- plus ``optimizer_state_dict``, which the reference's loader ignores and which makes a resume bitwise.
    ``phases``: the keys of ``step_img`` (train_SISR.py:330 keeps 'train' and one per noise type).  ``ema``: a ``WeightEMA``; the
    checkpoint then also holds ``ema_state_dict`` -- the averaged weights in the model's format, for :func:`load_model_state` -- and
    ``ema``: ``{"decay", "warmup", "num_updates"}``.  Callers that do not know the two keys ignore them."""
    out = {"epoch": int(epoch), "step": int(step), "step_img": {x: int(step_img[x]) for x in phases},
           "model_state_dict": net.state_dict()}
    if opt is not None:
        out["optimizer_state_dict"] = opt.state_dict()
    if ema is not None:
        out["ema_state_dict"] = ema.model_state_dict()
        out["ema"] = {"decay": ema.decay, "warmup": ema.warmup, "num_updates": ema.num_updates}
    return out


def model_state_of(ckpt: dict, ema: bool = False) -> dict:
    """The weights of a checkpoint: ``model_state_dict`` (the last iterate) or, with ``ema``, ``ema_state_dict`` (the averaged weights of a
    run with ``ema_decay``); ``KeyError`` naming the key when the checkpoint has none."""
    key = "ema_state_dict" if ema else "model_state_dict"
    if key not in ckpt:
        raise KeyError(f"checkpoint lacks {key!r}" + (": it was written by a run without ema_decay" if ema else ""))
    return ckpt[key]


def load_model_state(net: torch.nn.Module, state_dict: dict) -> None:
    """``net.load_state_dict`` that accepts the ``module.`` prefix a DistributedDataParallel checkpoint carries (testing_demo.py:69-72)."""
    if state_dict and all(k.startswith("module.") for k in state_dict):
        state_dict = {k[len("module."):]: v for k, v in state_dict.items()}
    net.load_state_dict(state_dict, strict=True)


def load_checkpoint(path, net: torch.nn.Module, opt: Optional[torch.optim.Optimizer] = None, map_location=None, ema=None) -> dict:
    """Load a checkpoint file (or an already loaded dict) into ``net`` and, when it holds one, the optimizer state into ``opt`` ->
    the checkpoint.  A reference checkpoint (no optimizer state) resumes with fresh Adam moments, as the reference itself does.
    ``ema``: a ``WeightEMA`` over ``net``'s parameters; it takes the checkpoint's averaged weights and update count (its own decay and
    warm-up setting stay: they are the run's configuration), or, from a checkpoint without them, starts again at the loaded parameters
    with ``num_updates = 0``."""
    ckpt = path if isinstance(path, dict) else torch.load(os.fspath(path), map_location=map_location)
    for key in ("epoch", "model_state_dict"):
        if key not in ckpt:
            raise KeyError(f"checkpoint lacks {key!r}")
    load_model_state(net, ckpt["model_state_dict"])
    if opt is not None and ckpt.get("optimizer_state_dict") is not None:
        opt.load_state_dict(ckpt["optimizer_state_dict"])
    if ema is not None:
        _restore_ema(ckpt, ema)
    return ckpt


def _restore_ema(ckpt: dict, ema) -> None:
    """The checkpoint's averaged weights and update count into ``ema``, whose parameters already hold the checkpoint's; without the two
    keys the shadows start at those parameters."""
    have = ckpt.get("ema_state_dict") is not None and ckpt.get("ema") is not None
    shadow = ckpt["ema_state_dict"] if have else {n: p.detach() for n, p in zip(ema.names, ema.params)}
    ema.load_state_dict({"decay": ema.decay, "warmup": ema.warmup, "num_updates": int(ckpt["ema"]["num_updates"]) if have else 0,
                         "shadow": shadow})


# ---- the reference's log lines ---------------------------------------------------------------------------------------------------------------
def train_line(epoch: int, epochs: int, ii: int, num_iter: int, row: Sequence[float], clip_r: float, clip_s: float, lr: float) -> str:
    """train_denoising_syn.py:194-198 for step ``ii`` (0-based) from its log row (Loss, lh, KLG, KLIG, GNorm_R, GNorm_S)."""
    _, lh, klg, klig, norm_r, norm_s = (float(v) for v in row)
    return (f"[Epoch:{epoch + 1:>2d}/{epochs:<2d}] train:{ii + 1:0>5d}/{num_iter:0>5d}, lh={lh:+4.2f}, KLG={klg:+>7.2f}, KLIG={klig:+>6.2f}, "
            f"GNorm_D:{clip_r:.1e}/{norm_r:.1e}, GNorm_S:{clip_s:.1e}/{norm_s:.1e}, lr={lr:.2e}")


def epoch_line(sums: Sequence[float]) -> str:
    """train_denoising_syn.py:215-217 from the epoch's running sums."""
    return f"train: Loss={sums[0]:+.2e}, lh={sums[1]:+.2e}, KL_Guass={sums[2]:+.2e}, KLIG={sums[3]:+.2e}"


def sisr_train_line(epoch: int, epochs: int, ii: int, num_iter: int, row: Sequence[float], lr: float) -> str:
    """train_SISR.py:239-243 for step ``ii`` (0-based) from its log row (Loss, lh, KLR, KLS, KLK, GNorm_R, GNorm_S, GNorm_K)."""
    _, lh, klr, kls, klk, norm_r, norm_s, norm_k = (float(v) for v in row)
    return (f"[Epoch:{epoch + 1:>3d}/{epochs:<3d}] train:{ii + 1:0>5d}/{num_iter:0>5d}, lh:{lh:+>5.2f}, KL:{klr:+>7.2f}/{kls:+>6.2f}/{klk:+>6.2f}, "
            f"Grad:{norm_r:.1e}/{norm_s:.1e}/{norm_k:.1e}, lr={lr:.1e}")


def sisr_epoch_line(sums: Sequence[float]) -> str:
    """train_SISR.py:267-269 from the epoch's running sums."""
    return f"train: Loss={sums[0]:+.2e}, lh={sums[1]:>4.2f}, KLR={sums[2]:+>7.2f}, KLS={sums[3]:+>6.2f}, KLK={sums[4]:+>5.2f}"


def sisr_test_line(noise_type: str, epoch: int, epochs: int, ii: int, num_test: int, psnr: float, ssim: float) -> str:
    """train_SISR.py:291-293 for test image ``ii`` (0-based; the reference prints every third)."""
    return f"Noise: {noise_type:s}, Epoch:{epoch + 1:>3d}/{epochs:<3d}] test:{ii + 1:0>3d}/{num_test:0>3d}, psnr={psnr:4.2f}, ssim={ssim:5.4f}"


def sisr_summary_line(noise_type: str, psnr: float, ssim: float) -> str:
    """train_SISR.py:319-320."""
    return f"Noise: {noise_type:s}, test: PSNR={psnr:4.2f}, SSIM={ssim:5.4f}"


# ---- validation ------------------------------------------------------------------------------------------------------------------------------
def _check_val(val, real: bool, device: torch.device):
    if val is None:
        return
    if real:
        if not isinstance(val, datagen.ImagePool) or val.data_b is None:
            raise TypeError("val: the real-noise loop validates on a paired pool of equal-size blocks (ImagePool.paired)")
        h, w = val.shapes[0]
        if h != w or any(s != (h, w) for s in val.shapes):
            raise ValueError("val: the blocks of the paired validation pool must be square and of one size")
        dev = val.device
    else:
        if not isinstance(val, datagen.SimulateTestSet):
            raise TypeError(f"val must be a datagen.SimulateTestSet, got {type(val).__name__}")
        dev = val.pool.device
    if dev != device:
        raise RuntimeError(f"val is on {dev}, the training pool on {device}")


def _sisr_val_sets(val, c: dict, device: torch.device) -> Dict[str, "datagen.GeneralTestSet"]:
    if val is None:
        return {}
    sets = {val.noise_type: val} if isinstance(val, datagen.GeneralTestSet) else val
    if not isinstance(sets, dict) or not sets:
        raise TypeError("val must be a datagen.GeneralTestSet or a dict {noise type: GeneralTestSet}")
    for key, vs in sets.items():
        if key not in NOISE_TYPES:
            raise ValueError(f"val: noise type {key!r}: one of {NOISE_TYPES} is expected")
        if not isinstance(vs, datagen.GeneralTestSet):
            raise TypeError(f"val[{key!r}] must be a datagen.GeneralTestSet, got {type(vs).__name__}")
        if vs.noise_type != key:
            raise ValueError(f"val[{key!r}] was built with noise_type={vs.noise_type!r}")
        if vs.sf != c["sf"]:
            raise ValueError(f"val[{key!r}] was built for sf {vs.sf}, the loop trains sf {c['sf']}")
        if vs.pool.device != device:
            raise RuntimeError(f"val[{key!r}] is on {vs.pool.device}, the training pool on {device}")
    return dict(sets)


def _validate(net: torch.nn.Module, groups: Sequence[Sequence[int]], fetch: Callable, forward: Callable, metric: Callable,
              on_batch: Optional[Callable] = None) -> Tuple[List[float], List[float]]:
    """A test stage: per chunk of ``VAL_BATCH`` indices of a same-shape group, ``fetch(idx) -> (input, ground truth)``, the un-clipped
    ``mu`` of ``forward(input)`` into ``metric(mu, ground truth)`` (a ``metrics.psnr_ssim`` call: clip, quantisation, PSNR and SSIM on the
    device), and ONE ``metrics.to_floats`` for the whole set -> (per-image PSNR, per-image SSIM) in image order.  ``on_batch(idx, input,
    ground truth, forward's result)``: called per chunk after its metric, inside the stage's ``no_grad``; it must not synchronise."""
    was_training = net.training
    net.eval()
    pending, order = [], []
    try:
        with torch.no_grad():
            for group in groups:
                for k in range(0, len(group), VAL_BATCH):
                    idx = group[k:k + VAL_BATCH]
                    im_in, im_gt = fetch(idx)
                    result = forward(im_in)
                    mu = result[0]
                    mu = mu[0] if isinstance(mu, (list, tuple)) else mu
                    pending.append(metric(mu, im_gt))
                    order += idx
                    if on_batch is not None:
                        on_batch(idx, im_in, im_gt, result)
        psnrs, ssims = metrics.to_floats(*(torch.cat(col) for col in zip(*pending)))
    finally:
        net.train(was_training)
    back = np.argsort(np.asarray(order), kind="stable")
    return [psnrs[i] for i in back], [ssims[i] for i in back]


def validate(net: torch.nn.Module, val, real: bool = False, on_batch: Optional[Callable] = None) -> Tuple[List[float], List[float]]:
    """The test stage (train_denoising_syn.py:222-257, train_denoising_real.py:214-247) as :func:`_validate` runs it, on a
    ``SimulateTestSet`` or, for ``real``, on the uncropped blocks of a paired pool.  ``on_batch(idx, im_noisy, im_gt, (mu, sigma))``: per
    chunk of images (:func:`_validate`)."""
    if real:
        p = val.shapes[0][0]

        def fetch(idx):
            zeros = [0] * len(idx)
            return datagen.pair_batch(val, datagen.BatchParams(val.shapes, p, idx, zeros, zeros, zeros), p)
        groups = [list(range(len(val)))]
    else:
        fetch, groups = val.batch, val.groups()
    return _validate(net, groups, fetch, net, lambda mu, im_gt: metrics.psnr_ssim(mu[:, :im_gt.shape[1]], im_gt), on_batch)


def validate_sisr(net: torch.nn.Module, val: "datagen.GeneralTestSet", sf: int, on_batch: Optional[Callable] = None) -> Tuple[List[float], List[float]]:
    """The test stage for one noise type (train_SISR.py:279-288) as :func:`_validate` runs it, with
    ``metrics.psnr_ssim(mu, im_hr, border=sf**2, ycbcr="float")`` -- ``util_image.batch_PSNR / batch_SSIM(..., sf**2, True)`` on the device.
    ``on_batch(idx, im_lr, im_hr, (mu, kinfo_est, sigma_est), kinfo_gt)``: per chunk of images (:func:`_validate`)."""
    last = {}

    def fetch(idx):
        im_hr, im_lr, last["kinfo_gt"] = val.batch(idx)
        return im_lr, im_hr
    chunk = None if on_batch is None else (lambda idx, im_lr, im_hr, result: on_batch(idx, im_lr, im_hr, result, last["kinfo_gt"]))
    return _validate(net, val.groups(), fetch, lambda im_lr: net(im_lr, sf), lambda mu, im_hr: metrics.psnr_ssim(mu, im_hr, border=sf ** 2, ycbcr="float"),
                     chunk)


# ---- the steps -------------------------------------------------------------------------------------------------------------------------------
class Shard(NamedTuple):
    """A rank's part of a data-parallel step: rows ``[first, last)`` of the global batch and the reducer that averages its gradients."""
    world: int
    rank: int
    first: int
    last: int
    reducer: Optional[object] = None          # dist.GradientReducer


def shard_rows(batch: int, world: int, rank: int) -> Tuple[int, int]:
    """Rows [first, last) of the global batch that rank ``rank`` synthesises: ``dist.shard_range`` of a batch that the world divides
    (``batch // world`` rows each, as the reference's ``batch_size // num_gpus``)."""
    from .dist import shard_range
    if world < 1 or batch % world:
        raise ValueError(f"cfg['batch_size'] = {batch} is the global batch and must divide by the world size {world}")
    return shard_range(batch, world, rank)


def shard_real_params(params: "datagen.BatchParams", mix: "datagen.MixParams", first: int, last: int):
    """The real-noise batch of rows [first, last) as a batch of its own.  A row's MixUp partner may live on another rank, so the ``n = last
    - first`` rows are followed by their ``n`` partners, whose own partners are themselves: -> (parameters of the 2 n entries, their mix).
    The first ``n`` samples of ``real_batch`` on the pair are bit for bit rows [first, last) of the whole batch."""
    rows = np.arange(first, last)
    n = len(rows)
    partners = mix.perm[rows].astype(np.int64)
    index = np.concatenate([rows, partners])
    perm = np.concatenate([np.arange(n, 2 * n), np.arange(n, 2 * n)])
    return params.select(index), datagen.MixParams(perm, mix.lam[index])


def _average(shard: Optional[Shard], loss: Tensor) -> None:
    """``loss.backward()``, then exactly one averaging of the gradients over the ranks whichever route the backward took: the fused
    Function feeds the reducer itself, the per-conv route leaves ``p.grad`` for ``reduce_grads``."""
    if shard is None or shard.reducer is None:
        loss.backward()
        return
    shard.reducer.begin_step()
    loss.backward()
    shard.reducer.ensure_reduced()


def train_step(net, opt: ClipAdam, pool: datagen.ImagePool, c: dict, rng: random.Random, epoch: int, ii: int, alpha0: Tensor, real: bool,
               steplog: Optional[StepLog] = None, shard: Optional[Shard] = None, keep: Optional[dict] = None):
    """One step of the loop (train_denoising_syn.py:169-184 / train_denoising_real.py:160-177): batch, forward, objective, backward, clip
    and Adam step, and the push of the step's six scalars.  Nothing here synchronises.  -> (loss, lh, kl_g, kl_ig) on the device.
    ``shard``: the whole batch's parameters are drawn, the rank's rows synthesised and the gradients averaged before the clip.
    ``keep``: a dict that receives the step's own ``im_noisy``, ``im_gt``, ``sigma_gt``, ``mu`` and ``sigma`` (references, detached;
    nothing is copied or launched) for :func:`preview.denoise_train`."""
    b, p = c["batch_size"], c["patch_size"]
    if real:
        params, mix = datagen.draw_pair_params(rng, pool, b, p), datagen.draw_mixup_params(b)
        if shard is None:
            im_noisy, im_gt, sigma_gt = datagen.real_batch(pool, params, p, mix, k_size=c["var_window"])
        else:
            n = shard.last - shard.first
            params, mix = shard_real_params(params, mix, shard.first, shard.last)
            im_noisy, im_gt, _ = datagen.real_batch(pool, params, p, mix, k_size=None)
            im_noisy, im_gt = im_noisy[:n], im_gt[:n]
            sigma_gt = elbo.noise_estimate(im_noisy, im_gt, c["var_window"])
    else:
        params = datagen.draw_denoise_params(rng, pool, b, p)
        if shard is None:
            im_noisy, im_gt, sigma_gt = datagen.denoise_batch(pool, params, p, seed=epoch, base_id=ii * b)
        else:
            im_noisy, im_gt, sigma_gt = datagen.denoise_batch(pool, params.select(slice(shard.first, shard.last)), p, seed=epoch,
                                                              base_id=ii * b + shard.first)
    beta0 = alpha0 * sigma_gt
    opt.zero_grad()
    mu, sigma = net(im_noisy)
    loss, lh, kl_g, kl_ig = elbo.elbo_denoising(mu, sigma, im_noisy, im_gt, c["eps2"], alpha0, beta0)
    _average(shard, loss)
    opt.step()
    if steplog is not None:
        steplog.push(loss, lh, kl_g, kl_ig, opt.grad_norms)
    if keep is not None:
        keep.update(im_noisy=im_noisy, im_gt=im_gt, sigma_gt=sigma_gt, mu=[m.detach() for m in mu] if isinstance(mu, (list, tuple)) else mu.detach(),
                    sigma=sigma.detach())
    return loss, lh, kl_g, kl_ig


def sisr_train_step(net, opt: ClipAdam, pool: datagen.ImagePool, c: dict, rng: random.Random, epoch: int, ii: int, alpha0: Tensor, kappa0: Tensor,
                    steplog: Optional[StepLog] = None, shard: Optional[Shard] = None, keep: Optional[dict] = None):
    """One step of the SISR loop (train_SISR.py:197-229): batch, forward, objective, backward, the three clips and the Adam step, and the
    push of the step's eight scalars.  ``c``: :func:`read_sisr_config`'s dict.  The batch noise is drawn with ``seed = epoch * 1000`` and
    sample ids ``ii * batch_size + i``; ``elbo_sisr``'s draws come from torch's device generator.  Nothing here synchronises.
    -> (loss, [lh, kl_rnet, kl_snet, kl_knet, ...]) on the device.  ``shard``: as in :func:`train_step`.  ``keep``: a dict that receives
    the step's own ``im_hr``, ``im_lr``, ``kinfo_gt``, ``kinfo_est``, ``mu`` and ``kernel_resample`` (``detail[7]``, the kernel the
    objective sampled) for :func:`preview.sisr_train`; references, detached."""
    b, sf = c["batch_size"], c["sf"]
    params = datagen.draw_sisr_params(rng, pool, b, c["hr_size"], sf, c["noise_level"], c["add_jpeg"], c["noise_jpeg"])
    base_id = ii * b
    if shard is not None:
        params, base_id = params.select(slice(shard.first, shard.last)), base_id + shard.first
    im_hr, im_lr, im_blur, kinfo_gt, nlevel = datagen.sisr_batch(pool, params, c["hr_size"], sf, c["k_size"], seed=epoch * 1000,
                                                                 downsampler=c["downsampler"], shift=c["kernel_shift"], base_id=base_id)
    sigma_prior = elbo.noise_estimate(im_lr, im_blur, c["var_window"]) if c["add_jpeg"] else nlevel
    opt.zero_grad()
    mu, kinfo_est, sigma_est = net(im_lr, sf)
    loss, detail = elbo.elbo_sisr(mu=mu, sigma_est=sigma_est, kinfo_est=kinfo_est, im_hr=im_hr, im_lr=im_lr, sigma_prior=sigma_prior, alpha0=alpha0,
                                  kinfo_gt=kinfo_gt, kappa0=kappa0, r2=c["r2"], eps2=c["eps2"], sf=sf, k_size=c["k_size"], penalty_K=c["penalty_K"],
                                  downsampler=c["downsampler"], shift=c["kernel_shift"])
    _average(shard, loss)
    opt.step()
    if steplog is not None:
        steplog.push(loss, detail[0], detail[1], detail[2], detail[3], opt.grad_norms)
    if keep is not None:
        keep.update(im_hr=im_hr, im_lr=im_lr, kinfo_gt=kinfo_gt, kinfo_est=kinfo_est.detach(),
                    mu=[m.detach() for m in mu] if isinstance(mu, (list, tuple)) else mu.detach(), kernel_resample=detail[7])
    return loss, detail


# ---- the loop --------------------------------------------------------------------------------------------------------------------------------
def _denoise_train_preview(keep: dict):
    from . import preview
    return preview.denoise_train(keep, "train")


def _sisr_train_preview(keep: dict, c: dict):
    from . import preview
    return preview.sisr_train(keep, c, "train")


class _Task(NamedTuple):
    """What differs between the training loops; everything else is :func:`_fit`.  ``c`` below is the task's checked config."""
    name: str                              # in error messages
    log_names: Tuple[str, ...]             # the step log's columns ...
    n_means: int                           # ... of which the first n_means are the epoch means of ``out["train"]``
    lrs: List[float]                       # per epoch
    seed_scale: int                        # epoch e draws from random.Random(e * seed_scale) ...
    seed_torch: bool                       # ... and, if set, starts with torch.manual_seed(e * seed_scale)
    seed_rank: bool                        # ... after which rank r > 0 of a multi-rank job reseeds its device generator with e * seed_scale + r
    const_keys: Tuple[str, ...]            # the config's floats that the step takes as device constants after alpha0
    step: Callable                         # step(net, opt, pool, c, rng, epoch, ii, alpha0, *constants, steplog, keep=None): one training step
    clip_keys: Tuple[str, ...]             # the clip sets (:func:`_optimizer`)
    train_line: Callable                   # train_line(epoch, epochs, ii, num_iter, row, lr) -> str
    epoch_line: Callable                   # epoch_line(sums) -> str
    rule: int                              # the width of the rule after the epoch line
    phases: Tuple[str, ...]                # the keys of the checkpoint's ``step_img``
    results: dict                          # the return dictionary's empty "psnr", "ssim" and "val_images"
    test_stage: Callable                   # test_stage(net, epoch, epochs, out, log, writer, step_img): validate, log, append to those three
    preview_every: int                     # with a writer: a train event every so many print intervals ...
    train_preview: Callable                # ... train_preview(keep) -> (tags, grids) from what the step left in ``keep``


def _emit(writer, event: Tuple[List[str], list], step_img: Dict[str, int], key: str) -> None:
    """One preview event to the writer: its grids come to the host in ONE ``preview.to_host``, every image is written at
    ``step_img[key]``, which then advances."""
    from . import preview
    tags, grids = event
    for tag, image in zip(tags, preview.to_host(grids)):
        writer.add_image(tag, image, step_img[key], dataformats="HWC")
    step_img[key] += 1


class _TestPreviews:
    """The test previews of one stage: every ``every``-th image (1-based, as the reference's batch-1 loader counts) gets an event, built
    on the device inside the stage (:meth:`add`) and delivered in image order after the stage's own host read."""

    def __init__(self, every: int):
        self.every, self.queue = every, []

    def chosen(self, idx: Sequence[int]) -> List[Tuple[int, int]]:
        """(position in the chunk, image index) of the chunk's images that get an event"""
        return [(j, i) for j, i in enumerate(idx) if (i + 1) % self.every == 0]

    def add(self, image: int, event) -> None:
        self.queue.append((image, event))

    def deliver(self, writer, step_img: Dict[str, int], key: str) -> None:
        for _, event in sorted(self.queue, key=lambda item: item[0]):
            _emit(writer, event, step_img, key)
        self.queue = []


def _world(group) -> Tuple[int, int]:
    """(world size, rank) of the data-parallel job this process is a rank of; (1, 0) without an initialised process group."""
    import torch.distributed as tdist
    if not (tdist.is_available() and tdist.is_initialized()):
        return 1, 0
    return tdist.get_world_size(group), tdist.get_rank(group)


def _check_ranks_agree(net: torch.nn.Module, dev: torch.device, group, world: int, epoch: int, ema=None) -> None:
    """One fp64 checksum of all parameters per rank, formed on the device and gathered: identical averaged gradients give identical
    updates, so the ranks can only differ after a fault.  Raises ``RuntimeError`` naming the ranks that differ from rank 0.  ``ema``: the
    rank's ``WeightEMA``; the checksum of its averaged weights is compared as well (every rank keeps its own, nothing is communicated)."""
    import torch.distributed as tdist
    with torch.no_grad(), torch.cuda.device(dev):
        mine = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).double().sum().reshape(1)
        if ema is not None:
            mine = torch.cat([mine, ema.checksum()])
        sums = [torch.empty_like(mine) for _ in range(world)]
        tdist.all_gather(sums, mine, group=group)
        sums = torch.stack(sums).cpu().tolist()
    for k, what in enumerate(("parameters", "averaged weights")[:len(sums[0])]):
        off = [r for r in range(world) if not (sums[r][k] == sums[0][k])]
        if off:
            raise RuntimeError(f"{type(net).__name__}: after epoch {epoch + 1} the {what} of rank(s) {off} differ from rank 0's "
                               f"(checksums {[sums[r][k] for r in off]} against {sums[0][k]}): the ranks no longer train one model")


def _fit(task: _Task, net: torch.nn.Module, pool: datagen.ImagePool, c: dict, save_dir, resume, log: Callable[[str], None], group=None,
         writer=None) -> dict:
    """The loop of ``fit_denoising`` and ``fit_sisr``, after their argument checks."""
    from . import dist as vdist
    world, rank = _world(group)
    shard, own_reducer = None, False
    if world > 1:
        first, last = shard_rows(c["batch_size"], world, rank)
        reducer = None
        if isinstance(net, vdist.DistributedTrainer):          # the wrapper's reducer is reused, the loop runs the module itself
            net, reducer = net.module, net.reducer
    dev = datagen._require_device(pool.device, task.name)
    for name, prm in net.named_parameters():
        if prm.device != dev:
            raise RuntimeError(f"{task.name}: parameter {name} is on {prm.device}, the pool on {dev}")
    epochs, num_iter = c["epochs"], c["steps_per_epoch"]
    opt = _optimizer(net, c, task.clip_keys)
    epoch_start, step, step_img = 0, 0, {x: 0 for x in task.phases}
    if world > 1 and rank != 0:
        log, save_dir, writer = (lambda line: None), None, None          # rank 0 prints, validates, saves and writes summaries (train_denoising_syn.py:186, 222, 260)
    ckpt = None
    if resume:
        ckpt = load_checkpoint(resume, net, opt, map_location=dev)
        epoch_start, step = int(ckpt["epoch"]), int(ckpt.get("step", 0))
        step_img = {x: int(ckpt.get("step_img", {}).get(x, 0)) for x in task.phases}
        log(f"=> Loaded checkpoint {resume if not isinstance(resume, dict) else '<dict>'} (epoch {epoch_start:d})")
    if world > 1:
        if not resume:
            vdist.broadcast_parameters(net, 0, group=group)
        if reducer is None:
            reducer, own_reducer = vdist.GradientReducer(net.parameters(), group=group), True
            net._grad_reducer = reducer                        # the fused backward feeds it (train.DenoiseFunction.backward)
        shard = Shard(world, rank, first, last, reducer)
    ema = None
    if c.get("ema_decay"):                                     # after the resume / broadcast: the shadows start at the parameters trained from
        from .ema import WeightEMA
        ema = WeightEMA(net, decay=c["ema_decay"], warmup=c["ema_warmup"])
        if ckpt is not None:
            _restore_ema(ckpt, ema)
        log(f"=> Weight average: decay {ema.decay:g}{' with warm-up' if ema.warmup else ''}, {ema.num_updates:d} updates so far; "
            f"validation uses the averaged weights")
    model_dir = None
    if save_dir is not None:
        model_dir = os.path.join(os.fspath(save_dir), "models")
        os.makedirs(model_dir, exist_ok=True)
    with torch.cuda.device(dev):
        alpha0 = (0.5 * torch.tensor([c["var_window"] ** 2], dtype=torch.float32)).to(dev)
        consts = [torch.tensor([c[k]], dtype=torch.float32).to(dev) for k in task.const_keys]
    steplog = StepLog(task.log_names, max(1, min(c["print_freq"], num_iter)), num_iter, dev)
    out = {"epoch_start": epoch_start, "lr": [], "train": [], **task.results, "checkpoints": [], "optimizer": opt}
    if ema is not None:
        out["ema"] = ema
    rows: List[np.ndarray] = []
    extra = {} if shard is None else {"shard": shard}
    try:
        for epoch in range(epoch_start, epochs):
            tic = time.time()
            rng = random.Random(epoch * task.seed_scale)
            if task.seed_torch:
                torch.manual_seed(epoch * task.seed_scale)
                if task.seed_rank and rank > 0:                # every rank its own device draws; rank 0 keeps the one-process stream
                    torch.cuda.default_generators[dev.index].manual_seed(epoch * task.seed_scale + rank)
            lr = task.lrs[epoch]
            for pgroup in opt.param_groups:
                pgroup["lr"] = lr
            net.train()
            steplog.reset()
            sums = np.zeros(len(task.log_names))
            with torch.cuda.device(dev):
                for ii in range(num_iter):
                    keep = {} if writer is not None and (ii + 1) % (task.preview_every * c["print_freq"]) == 0 else None
                    if keep is None:
                        task.step(net, opt, pool, c, rng, epoch, ii, alpha0, *consts, steplog, **extra)
                    else:
                        task.step(net, opt, pool, c, rng, epoch, ii, alpha0, *consts, steplog, keep=keep, **extra)
                    if ema is not None:
                        ema.update()
                    show = (ii + 1) % c["print_freq"] == 0 or ii == 0
                    if show or ii == num_iter - 1:
                        new, sums = steplog.read()          # the loop's only host read
                        rows.append(new)
                        if show:
                            log(task.train_line(epoch, epochs, ii, num_iter, new[-1], lr))
                            if writer is not None:
                                writer.add_scalar("Train Loss Iter", float(new[-1][0]), step)
                            step += 1
                    if keep is not None:                    # (a multiple of print_freq: the log was read just above)
                        _emit(writer, task.train_preview(keep), step_img, "train")
            if shard is not None:
                _check_ranks_agree(net, dev, group, world, epoch, ema)
            log(task.epoch_line(sums))
            if writer is not None:
                writer.add_scalar("Loss_epoch", float(sums[0]), epoch)
            log("-" * task.rule)
            out["lr"].append(lr)
            out["train"].append({k: float(v) for k, v in zip(task.log_names[:task.n_means], sums[:task.n_means])})
            if rank == 0:
                with torch.cuda.device(dev):
                    if ema is None:
                        task.test_stage(net, epoch, epochs, out, log, writer, step_img)
                    else:
                        with ema.averaged():
                            task.test_stage(net, epoch, epochs, out, log, writer, step_img)
            if model_dir is not None:
                path = os.path.join(model_dir, f"model_{epoch + 1}.pth")
                torch.save(checkpoint_dict(net, opt, epoch + 1, step + 1, step_img, task.phases, ema), path)
                out["checkpoints"].append(path)
            log(f"This epoch take time {time.time() - tic:.2f}")
    finally:
        if own_reducer:
            del net._grad_reducer
    out["rows"] = np.concatenate(rows) if rows else np.zeros((0, len(task.log_names)), dtype=np.float32)
    out["step"], out["step_img"] = step, step_img
    out["world"], out["rank"] = world, rank
    return out


def fit_denoising(net: torch.nn.Module, pool: datagen.ImagePool, cfg: dict, *, val=None, real: bool = False, save_dir=None, resume=None,
                  log: Callable[[str], None] = print, group=None, writer=None) -> dict:
    """Train ``net`` (a ``VIRAttResUNet`` on the pool's device) as train_denoising_syn.py does, or with ``real=True`` -- ``pool`` then built
    by ``ImagePool.paired`` -- as train_denoising_real.py does.

    ``cfg``: the reference's keys ``batch_size, patch_size, epochs, warmup_epochs, lr, lr_min, print_freq, clip_grad_R, clip_grad_S,
    var_window, eps2`` plus ``steps_per_epoch`` (default 10000, the reference's dataset length over its batch size).  ``val``: a
    ``datagen.SimulateTestSet`` (or, for ``real``, a paired pool of equal-size square blocks): the test stage runs after every epoch.
    ``save_dir``: ``<save_dir>/models/model_<epoch>.pth`` is written after every epoch in the reference's format plus the optimizer
    state.  ``resume``: such a file (or a reference checkpoint; a ``module.`` prefix on its keys is accepted); training continues at
    ``checkpoint['epoch']``.  ``log``: receives every line the reference prints.  ``group``: the process group of a data-parallel job
    (None: the default group); with ``torch.distributed`` initialised and more than one rank the call is ONE RANK of the job (module
    docstring: ``batch_size`` is the global batch, rank 0 logs, validates and saves); with one process nothing changes.

    Weight average (off by default): with ``cfg["ema_decay"]`` in (0, 1) -- and optionally ``cfg["ema_warmup"]`` -- a ``ema.WeightEMA`` of
    the parameters is updated after every step, the test stage runs on the averaged weights, the checkpoint gains ``ema_state_dict``
    (model format, :func:`model_state_of`) and ``ema``, a resume restores both, every rank keeps its own shadows, and the returned
    dictionary gains ``"ema"``.  The live parameters, the Adam state and ``rows`` are those of the run without it, bit for bit.

    ``writer`` (default None: nothing below happens and ``step_img`` stays at zero): a summary writer -- ``preview.FolderWriter``,
    ``torch.utils.tensorboard.SummaryWriter``, tensorboardX; ``add_scalar(tag, float, step)`` and ``add_image(tag, uint8 [H, W, 3], step,
    dataformats="HWC")`` are all that is called, on rank 0 only.  It receives what the reference writes: ``'Train Loss Iter'`` at every
    printed step, ``'Loss_epoch'``, after the test stage ``'PSNR_epoch_test'`` / ``'SSIM_epoch_test'`` (not without ``val``), the five
    train grids (:func:`preview.denoise_train`) at every step with ``(ii + 1) % (PREVIEW_EVERY * print_freq) == 0`` and the four test
    grids (:func:`preview.denoise_test`) of every ``TEST_PREVIEW_EVERY``-th validation image, numbered by ``step_img``, which the
    checkpoint carries.  The grids are formed on the device from tensors the step already has and come to the host in one copy per
    event; parameters, Adam state, ``rows`` and the random streams are those of the run without a writer, bit for bit.

    Returns ``{"epoch_start", "lr": [...], "train": [{"Loss", "lh", "KLG", "KLIG"} per epoch: the reference's epoch means], "psnr": [...],
    "ssim": [...] (per epoch, NaN without ``val``), "val_images": [(per-image PSNR, per-image SSIM) per epoch], "rows": float32 [steps, 6] (every step's Loss, lh, KLG, KLIG and the two pre-clip
    gradient norms), "step", "step_img", "checkpoints": [paths], "optimizer", "world", "rank"}``."""
    c = read_config(cfg)
    if not isinstance(pool, datagen.ImagePool):
        raise TypeError(f"pool must be a datagen.ImagePool, got {type(pool).__name__}")
    if real and pool.data_b is None:
        raise ValueError("real=True: the pool has no second buffer; build it with ImagePool.paired")
    dev = datagen._require_device(pool.device, "fit_denoising")
    _check_val(val, real, dev)

    def test_stage(net, epoch, epochs, out, log, writer, step_img):
        psnr = ssim = float("nan")
        if val is not None:
            shots = on_batch = None
            if writer is not None:
                from . import preview

                def on_batch(idx, im_noisy, im_gt, result):
                    mu = result[0][0] if isinstance(result[0], (list, tuple)) else result[0]
                    for j, i in shots.chosen(idx):
                        shots.add(i, preview.denoise_test(mu[j:j + 1], im_gt[j:j + 1], result[1][j:j + 1], im_noisy[j:j + 1]))
                shots = _TestPreviews(TEST_PREVIEW_EVERY)
            psnrs, ssims = validate(net, val, real, on_batch)
            psnr, ssim = float(np.mean(psnrs)), float(np.mean(ssims))
            out["val_images"].append((psnrs, ssims))
            log(f"test: PSNR={psnr:4.2f}, SSIM={ssim:5.4f}")
            log("-" * 90)
            if writer is not None:
                shots.deliver(writer, step_img, "test")
                writer.add_scalar("PSNR_epoch_test", psnr, epoch)
                writer.add_scalar("SSIM_epoch_test", ssim, epoch)
        out["psnr"].append(psnr)
        out["ssim"].append(ssim)

    task = _Task(name="fit_denoising", log_names=LOG_NAMES, n_means=4, lrs=warmup_cosine(c["lr"], c["lr_min"], c["epochs"], c["warmup_epochs"]),
                 seed_scale=1, seed_torch=real, seed_rank=False, const_keys=(), clip_keys=("rnet", "snet"),
                 step=lambda net, opt, pool, c, rng, epoch, ii, alpha0, steplog, **kw: train_step(net, opt, pool, c, rng, epoch, ii, alpha0, real, steplog, **kw),
                 train_line=lambda epoch, epochs, ii, num_iter, row, lr: train_line(epoch, epochs, ii, num_iter, row, c["clip_grad_R"], c["clip_grad_S"], lr),
                 epoch_line=epoch_line, rule=150, phases=("train", "test"), results={"psnr": [], "ssim": [], "val_images": []}, test_stage=test_stage,
                 preview_every=PREVIEW_EVERY, train_preview=_denoise_train_preview)
    return _fit(task, net, pool, c, save_dir, resume, log, group, writer)


def fit_sisr(net: torch.nn.Module, pool: datagen.ImagePool, cfg: dict, *, val=None, save_dir=None, resume=None,
             log: Callable[[str], None] = print, group=None, writer=None) -> dict:
    """Train ``net`` (a ``VIRAttResUNetSR`` on the pool's device) as train_SISR.py does, in one process or as one rank of a
    data-parallel job (``group``, as in :func:`fit_denoising`; rank r > 0 reseeds its device generator with ``e * 1000 + r``).

    ``cfg``: the reference's keys as they stand in configs/sisr_x*.json (:func:`read_sisr_config`; the booleans are the strings "True" /
    "False") plus ``steps_per_epoch`` (default 10000).  ``net.noise_avg`` must equal ``not add_jpeg`` (:87).  ``val``: a
    ``datagen.GeneralTestSet`` or a dict ``{noise type: set}``: the test stage runs after every epoch, per noise type.  ``save_dir``,
    ``resume``, ``log``: as in :func:`fit_denoising`; the checkpoint's ``step_img`` has the keys 'train' and one per noise type (:330).

    Per epoch ``e``: ``random.Random(e * 1000)`` draws the batch parameters and ``torch.manual_seed(e * 1000)`` seeds the generators
    (``GeneralTrainFloder.reset_seed``, which in the reference's main process also reseeds the device generator that ``elbo_sisr`` draws
    from); the learning rate is ``schedule.cosine(lr, lr_min, epochs)[e]``.  The host reads the step log at the first step, at every
    ``print_freq``-th step and at the end of the epoch.  ``ema_decay`` / ``ema_warmup``: the weight average, as in :func:`fit_denoising`.
    ``writer``: a summary writer, as in :func:`fit_denoising`; it receives ``'Train Loss Iter'``, ``'Loss_epoch'``, per noise type
    ``'<noise type> PSNR Test'`` / ``'<noise type> SSIM Test'``, the six train grids (:func:`preview.sisr_train`) at every step with
    ``(ii + 1) % (SISR_PREVIEW_EVERY * print_freq) == 0`` and the five test grids (:func:`preview.sisr_test`) of every
    ``SISR_TEST_PREVIEW_EVERY``-th validation image, numbered by ``step_img['train']`` and ``step_img[noise type]``.

    Returns ``{"epoch_start", "lr": [...], "train": [{"Loss", "lh", "KLR", "KLS", "KLK"} per epoch: the reference's epoch means], "psnr":
    {noise type: [...]}, "ssim": {noise type: [...]} (per epoch), "val_images": {noise type: [(per-image PSNR, per-image SSIM) per
    epoch]}, "rows": float32 [steps, 8] (every step's Loss, lh, KLR, KLS, KLK and the three pre-clip gradient norms), "step", "step_img",
    "checkpoints": [paths], "optimizer", "world", "rank"}``."""
    c = read_sisr_config(cfg)
    if not isinstance(pool, datagen.ImagePool):
        raise TypeError(f"pool must be a datagen.ImagePool, got {type(pool).__name__}")
    if not hasattr(net, "noise_avg") or bool(net.noise_avg) != (not c["add_jpeg"]):
        raise ValueError(f"fit_sisr: add_jpeg={c['add_jpeg']} needs a network built with noise_avg={not c['add_jpeg']} (train_SISR.py:87), "
                         f"got noise_avg={getattr(net, 'noise_avg', None)}")
    dev = datagen._require_device(pool.device, "fit_sisr")
    vals = _sisr_val_sets(val, c, dev)
    noise_types = {"Gaussian", "JPEG"} if c["add_jpeg"] else {"Gaussian"}

    def test_stage(net, epoch, epochs, out, log, writer, step_img):
        for noise_type, vs in vals.items():
            shots = on_batch = None
            if writer is not None:
                from . import preview

                def on_batch(idx, im_lr, im_hr, result, kinfo_gt, noise_type=noise_type):
                    mu = result[0][0] if isinstance(result[0], (list, tuple)) else result[0]
                    for j, i in shots.chosen(idx):
                        shots.add(i, preview.sisr_test(mu[j:j + 1], im_hr[j:j + 1], im_lr[j:j + 1], kinfo_gt[j:j + 1], result[1][j:j + 1], c, noise_type))
                shots = _TestPreviews(SISR_TEST_PREVIEW_EVERY)
            psnrs, ssims = validate_sisr(net, vs, c["sf"], on_batch)
            psnr = ssim = 0                               # (:278-288, 315-316: a running sum in image order, then one division)
            for ii, (p_i, s_i) in enumerate(zip(psnrs, ssims)):
                psnr += p_i
                ssim += s_i
                if (ii + 1) % 3 == 0:
                    log(sisr_test_line(noise_type, epoch, epochs, ii, len(vs), p_i, s_i))
            psnr, ssim = psnr / len(psnrs), ssim / len(ssims)
            out["val_images"][noise_type].append((psnrs, ssims))
            out["psnr"][noise_type].append(float(psnr))
            out["ssim"][noise_type].append(float(ssim))
            if writer is not None:
                shots.deliver(writer, step_img, noise_type)
                writer.add_scalar(noise_type + " PSNR Test", float(psnr), epoch)
                writer.add_scalar(noise_type + " SSIM Test", float(ssim), epoch)
            log(sisr_summary_line(noise_type, psnr, ssim))
            log("-" * 60)

    task = _Task(name="fit_sisr", log_names=SISR_LOG_NAMES, n_means=5, lrs=cosine(c["lr"], c["lr_min"], c["epochs"]), seed_scale=1000, seed_torch=True,
                 seed_rank=True, const_keys=("kappa0",), step=sisr_train_step, clip_keys=("rnet", "snet", "knet"), train_line=sisr_train_line, epoch_line=sisr_epoch_line, rule=105,
                 phases=("train",) + tuple(sorted(noise_types | set(vals), key=NOISE_TYPES.index)),
                 results={"psnr": {x: [] for x in vals}, "ssim": {x: [] for x in vals}, "val_images": {x: [] for x in vals}}, test_stage=test_stage,
                 preview_every=SISR_PREVIEW_EVERY, train_preview=lambda keep: _sisr_train_preview(keep, c))
    return _fit(task, net, pool, c, save_dir, resume, log, group, writer)
