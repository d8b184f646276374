"""TrainUnifiedVideoActionWorkspace: the reference's training loop
(workspace/train_unified_video_action_workspace.py:41-422), selected by `model._target_`
(config/model/uva.yaml:1) and run by train.py (`cls(cfg).run()`, train.py:58-60).

Same structure and order:
  __init__ (:44-79)   seed torch / numpy / random = training.seed on every rank; instantiate
                      model.policy with task_name / task_modes / normalizer_type /
                      language_emb_model; ema_model = deepcopy(model); optimizer =
                      model.get_optimizer(**model.policy.optimizer).
  run (:82-422)       dataloaders (DataLoader(dataset, **dataloader), rank-sharded), normalizer
                      from the dataset on rank 0 -> every rank, lr scheduler (get_scheduler,
                      num_training_steps = len(dl) * num_epochs // grad_accum,
                      last_epoch = global_step - 1), resume from latest.ckpt, EMAModel via
                      `ema._target_`, debug overrides (:222-229), then per batch:
                        device transfer -> model(batch) -> backward -> optimizer.step ->
                        zero_grad -> lr_scheduler.step -> ema.step(model) -> step log
                      and per epoch the checkpoint (latest + top-k on rank 0).
MI355X differences (results unchanged):
  * no accelerate / DDP wrapper: one process per GPU (torchrun or `accelerate launch` env),
    torch.distributed over RCCL; the optimizer's bucket reducer all-reduces the flat gradient
    buffer from inside backward (workspace/optim.GradReducer) and the AdamW kernel averages.
  * `mixed_precision` fp16 / bf16 -> bf16 MFMA operands with fp32 accumulation, residual
    streams and master weights (no GradScaler needed); "no" -> fp32.
  * the frame resize runs inside the policy (fused with frame selection), so the workspace
    does not call resize_image.
  * step logs are read back one step late (a pinned host copy + event instead of three
    blocking .item() calls), so the host keeps queueing the next step.
  * the epoch-end evaluation (workspace:342-376 -> eval/eval.py) runs on rank 0, on the EMA policy when
    training.use_ema, in the reference's order and under its conditions, but only when asked for: FVD
    (predict_video) when training.i3d_pretrained_path names a local I3D weight file (nothing is
    downloaded; training.fvd_precision fp32 | bf16, default fp32), action L2 (predict_action, no
    env_runner) when training.eval_action_l2 is true.  Their keys (video_fvd,
    val_action_l2_distances) reach the top-k manager; env rollouts stay out of scope, and
    the top-k monitor still falls back to train_loss while its configured key is absent.
"""
import copy
import json
import os
import random

import numpy as np
import torch
import torch.distributed as dist

from .. import config as C
from ..runtime import RT
from .base_workspace import BaseWorkspace
from ..utils.augment import augment_batch
from ..utils.prefetch import PinnedPrefetcher


def dist_env():
    """(world, rank, local_rank) from torchrun / accelerate-launch environment variables."""
    return (int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")),
            int(os.environ.get("LOCAL_RANK", "0")))


def init_distributed(device_type="cuda"):
    world, rank, local = dist_env()
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if device_type == "cuda":
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
    return world, rank, local


def _to_device(x, dev):
    if isinstance(x, dict):
        return {k: _to_device(v, dev) for k, v in x.items()}
    return x.to(dev, non_blocking=True) if torch.is_tensor(x) else x


class TopKCheckpointManager:
    """common/checkpoint_util.py:5-60."""

    FALLBACK = ("train_loss", "min", "epoch={epoch:04d}-train_loss={train_loss:.3f}.ckpt")

    def __init__(self, save_dir, monitor_key, mode="min", k=1, format_str="epoch={epoch:03d}.ckpt"):
        assert mode in ("max", "min") and k >= 0
        self.save_dir, self.monitor_key, self.mode, self.k, self.format_str = save_dir, monitor_key, mode, k, format_str
        self.maps = {monitor_key: {}}  # ranking key -> {path: value}
        self.path_value_map = self.maps[monitor_key]

    def get_ckpt_path(self, data):
        if self.k == 0:
            return None
        if self.monitor_key in data:
            key, mode, fmt = self.monitor_key, self.mode, self.format_str
        else:
            # Difference from the reference (which raises KeyError): test_mean_score comes from env-runner
            # rollouts this workspace does not run, and video_fvd / val_action_l2_distances / video_psnr /
            # video_ssim are logged only when the epoch-end evaluation is switched on (training.i3d_pretrained_path
            # / training.eval_action_l2 / training.eval_video_metrics), so a call without the configured key ranks by train_loss (min)
            # under a file name that says so -- per call, in a ranking of its own: the configured key,
            # once logged, is used again
            if self.FALLBACK[0] not in data:
                return None
            key, mode, fmt = self.FALLBACK
            if key not in self.maps:
                print(f"TopKCheckpointManager: '{self.monitor_key}' is not logged by this workspace; "
                      f"ranking top-k checkpoints by {key} ({mode}) while it is absent")
        pv = self.maps.setdefault(key, {})
        value = data[key]
        path = os.path.join(self.save_dir, fmt.format(**data))
        if len(pv) < self.k:
            pv[path] = value
            return path
        ranked = sorted(pv.items(), key=lambda x: x[1])
        drop = None
        if mode == "max" and value > ranked[0][1]:
            drop = ranked[0][0]
        elif mode == "min" and value < ranked[-1][1]:
            drop = ranked[-1][0]
        if drop is None:
            return None
        del pv[drop]
        pv[path] = value
        if os.path.exists(drop):
            os.remove(drop)
        return path


class _LaggedLog:
    """step values copied to pinned host memory behind an event; read one step later."""

    NAMES = ("train_loss", "diffusion_loss", "action_loss")

    def __init__(self):
        self.pending = None

    def push(self, tensors, meta, names=NAMES, record=None, decode=None):
        """tensors: one scalar device tensor per name.  record: an optional fp32 device vector that rides the
        same copy (the optimizer's gradient record); decode(list of its floats) -> further log entries."""
        dev = torch.stack([t.detach().float().reshape(()) for t in tensors])
        if record is not None:
            dev = torch.cat([dev, record.detach().float().reshape(-1)])
        host = torch.empty(dev.numel(), dtype=torch.float32, pin_memory=torch.cuda.is_available())
        host.copy_(dev, non_blocking=True)
        ev = None
        if dev.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        prev, self.pending = self.pending, (host, ev, meta, tuple(names), decode)
        return self._read(prev)

    def flush(self):
        prev, self.pending = self.pending, None
        return self._read(prev)

    @staticmethod
    def _read(item):
        if item is None:
            return None
        host, ev, meta, names, decode = item
        if ev is not None:
            ev.synchronize()
        vals = host.tolist()
        out = dict(meta)
        out.update(zip(names, vals))
        if decode is not None:
            out.update(decode(vals[len(names):]))
        return out


class TrainUnifiedVideoActionWorkspace(BaseWorkspace):
    include_keys = ["global_step", "epoch"]

    def __init__(self, cfg, output_dir=None):
        super().__init__(cfg, output_dir=output_dir)
        seed = cfg.training.seed
        torch.manual_seed(seed)
        np.random.seed(seed)
        random.seed(seed)
        RT.set_precision(_precision(cfg))
        language_emb_model = cfg.task.dataset.get("language_emb_model")
        if cfg.training.get("deepspeed_config") is not None:
            language_emb_model = None  # workspace:57-61
        self.model = C.instantiate(cfg.model.policy, task_name=cfg.task.name, task_modes=cfg.task.task_modes,
                                   normalizer_type=cfg.task.dataset.normalizer_type,
                                   language_emb_model=language_emb_model)
        self.ema_model = copy.deepcopy(self.model) if cfg.training.use_ema else None
        self.optimizer = self.model.get_optimizer(**cfg.model.policy.optimizer)
        # train_step calls optimizer.step() right after backward (no gradient reader between): the
        # DP tail all-reduce may overlap the AdamW of the already-reduced buckets.  Only with one
        # backward per step: under gradient accumulation the next micro-step's backward would write
        # the encoder-input gradients while their deferred all-reduce is still in flight
        if hasattr(self.optimizer, "overlap_tail"):
            self.optimizer.overlap_tail = int(cfg.training.get("gradient_accumulate_every", 1) or 1) == 1
        self._configure_grad_guard()
        self.global_step = 0
        self.epoch = 0

    # ---- gradient norm / clipping / non-finite guard (opt-in keys; off when all are absent) ---
    def grad_guard_on(self):
        t = self.cfg.training
        return t.get("max_grad_norm") is not None or bool(t.get("skip_nonfinite_steps", False)) or \
            bool(t.get("log_grad_norm", False))

    def _configure_grad_guard(self):
        """training.max_grad_norm / skip_nonfinite_steps / log_grad_norm -> the optimizer's guard, with the
        norm reported for the encoder, the decoder, the video heads, the action heads and the rest.
        (get_optimizer keeps the reference's signature, so the options are set after it.)"""
        self._skipped_logged = 0
        if not self.grad_guard_on():
            return
        if not hasattr(self.optimizer, "set_grad_guard"):
            raise RuntimeError("training.max_grad_norm / skip_nonfinite_steps / log_grad_norm need the flat-buffer "
                               "optimizer (FusedAdamWEMA)")
        t, m = self.cfg.training, self.model.model
        parts = {"encoder": [getattr(m, "encoder_blocks", None)], "decoder": [getattr(m, "decoder_blocks", None)],
                 "video_head": [getattr(m, "diffloss", None), getattr(m, "diffloss_wrist", None)],
                 "action_head": [getattr(m, "diffactloss", None), getattr(m, "diffproploss", None)]}
        mg = t.get("max_grad_norm")
        self.optimizer.set_grad_guard(max_grad_norm=None if mg is None else float(mg),
                                      skip_nonfinite=bool(t.get("skip_nonfinite_steps", False)), grad_norm_parts=parts)

    def _grad_log(self, vals):
        """the lagged gradient record -> log entries; skipped_steps counts the records seen so far"""
        from .optim import grad_stats_dict
        out = grad_stats_dict(vals, self.optimizer.grad_part_names)
        self._skipped_logged += out.pop("skipped")
        out["skipped_steps"] = self._skipped_logged
        return out

    # ---- setup (the part of run() before the loop) ------------------------------------------
    def setup(self, device=None):
        cfg = self.cfg
        self.world, self.rank, local = init_distributed("cuda" if torch.cuda.is_available() else "cpu")
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu"))
        self.dataset = C.instantiate(cfg.task.dataset)
        sampler = None
        dl_kw = dict(cfg.dataloader)
        if self.world > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(
                self.dataset, num_replicas=self.world, rank=self.rank, shuffle=bool(dl_kw.get("shuffle", False)),
                seed=cfg.training.seed)
            dl_kw.pop("shuffle", None)
        if not torch.cuda.is_available():
            dl_kw["pin_memory"] = False
        self.train_dataloader = torch.utils.data.DataLoader(self.dataset, sampler=sampler, **dl_kw)
        # normalizer: fitted on rank 0, its tensors broadcast to every rank (workspace:150-168)
        normalizer = self.dataset.get_normalizer()
        if self.world > 1:
            _broadcast_module_state(normalizer, self.device)
        self.model.set_normalizer(normalizer)
        if self.ema_model is not None:
            self.ema_model.set_normalizer(normalizer)
        from ..model.common.lr_scheduler import get_scheduler
        self.lr_scheduler = get_scheduler(
            cfg.training.lr_scheduler, optimizer=self.optimizer, num_warmup_steps=cfg.training.lr_warmup_steps,
            num_training_steps=(len(self.train_dataloader) * cfg.training.num_epochs)
            // cfg.training.gradient_accumulate_every,
            last_epoch=self.global_step - 1)
        if cfg.training.get("resume") and self.get_checkpoint_path().is_file():
            print(f"Resuming from checkpoint {self.get_checkpoint_path()}")
            self.load_checkpoint(path=self.get_checkpoint_path())
        self.model.to(self.device)
        if self.ema_model is not None:
            self.ema_model.to(self.device)
        # a fresh EMAModel after the (optional) resume, as the reference builds it (:190-193)
        self.ema = C.instantiate(cfg.ema, model=self.ema_model) if cfg.training.use_ema else None
        # debug overrides AFTER the LR schedule and the resume, in the reference's order
        # (workspace:172-234): the schedule keeps the full run's num_training_steps
        if cfg.training.debug:
            cfg.training.num_epochs = 2
            cfg.training.max_train_steps = 3
            cfg.training.max_val_steps = 3
            cfg.training.rollout_every = 1
            cfg.training.checkpoint_every = 1
            cfg.training.val_every = 1
            cfg.training.sample_every = 1
        self.model.train()
        # on-device training augmentation instead of the dataset workers' CPU one
        self.device_augment = bool(cfg.task.get("device_augment", False))
        # epoch-end evaluation (workspace:342-376), rank 0 only, off unless asked for
        self.val_dataloader, self.i3d = None, None
        run_fvd, run_l2 = self.eval_plan()
        if (run_fvd or run_l2 or self.eval_video_metrics()) and self.rank == 0:
            vkw = dict(cfg.val_dataloader)
            if not torch.cuda.is_available():
                vkw["pin_memory"] = False
            self.val_dataloader = torch.utils.data.DataLoader(self.dataset.get_validation_dataset(), **vkw)
            if run_fvd:
                from ..fvd.i3d import load_i3d_pretrained
                self.i3d = load_i3d_pretrained(cfg.training.i3d_pretrained_path, self.device,
                                               precision=cfg.training.get("fvd_precision", "fp32") or "fp32")
        return self

    # ---- epoch-end evaluation (workspace:342-376) ----------------------------------------------
    def eval_plan(self):
        """(run FVD, run action L2): the reference's conditions (predict_video; predict_action and no
        env_runner) AND this build's opt-in keys -- with both keys absent nothing is evaluated and an
        epoch logs what it always logged"""
        cfg = self.cfg
        pol = cfg.model.policy
        run_fvd = bool(pol.autoregressive_model_params.get("predict_video", True)) and \
            bool(cfg.training.get("i3d_pretrained_path"))
        run_l2 = bool(pol.action_model_params.predict_action) and "env_runner" not in cfg.task and \
            bool(cfg.training.get("eval_action_l2", False))
        return run_fvd, run_l2

    def eval_video_metrics(self):
        """the third decision, beside eval_plan()'s two: frame-wise PSNR / SSIM of the predicted future frames
        (eval/video_metrics.py) when the policy predicts video AND training.eval_video_metrics is set.  Needs no
        I3D weights: without training.i3d_pretrained_path no tower is built and only the metrics are logged"""
        cfg = self.cfg
        return bool(cfg.model.policy.autoregressive_model_params.get("predict_video", True)) and \
            bool(cfg.training.get("eval_video_metrics", False))

    def evaluate_epoch(self, rng=None):
        """-> the evaluation's log entries ({} when nothing is switched on or on a rank other than 0)"""
        run_fvd, run_l2 = self.eval_plan()
        run_vm = self.eval_video_metrics()
        if not (run_fvd or run_l2 or run_vm) or self.rank != 0:
            return {}
        from ..eval import eval as E
        cfg = self.cfg
        policy = self.ema_model if cfg.training.use_ema else self.model
        policy.eval()
        log = {}
        try:
            if run_vm:   # one pass of clip generation for the metrics and, when on, the FVD
                log.update(E.test_video_eval(cfg, policy, self.val_dataloader, self.epoch, self.output_dir,
                                             self.device, i3d=self.i3d, rng=rng, fvd=run_fvd, metrics=True))
            elif run_fvd:
                log.update(E.test_video_fvd(cfg, policy, self.val_dataloader, self.epoch, self.output_dir, self.device,
                                            i3d=self.i3d, rng=rng))
            if run_l2:
                log.update(E.test_action_l2(cfg, policy, self.val_dataloader, self.epoch, self.output_dir,
                                            self.device, rng=rng))
        finally:
            policy.train()
        return log

    # ---- one training step (workspace:279-302) -------------------------------------------------
    def train_step(self, batch, rng=None):
        """-> (raw_loss, diffusion_loss, action_loss) device tensors."""
        cfg = self.cfg
        raw_loss, (loss_diffusion, loss_action) = self.model(batch, rng=rng) if rng is not None else self.model(batch)
        raw_loss.backward()
        if self.global_step % cfg.training.gradient_accumulate_every == 0:
            self.optimizer.step()
            self.optimizer.zero_grad()
            self.lr_scheduler.step()
        if self.ema is not None:
            self.ema.step(self.model)
        return raw_loss, loss_diffusion, loss_action

    def run(self):
        cfg = self.cfg
        self.setup()
        topk = TopKCheckpointManager(save_dir=os.path.join(self.output_dir, "checkpoints"), **cfg.checkpoint.topk)
        os.makedirs(self.output_dir, exist_ok=True)
        log_path = os.path.join(self.output_dir, "logs.json.txt")
        logf = open(log_path, "a") if self.rank == 0 else None
        lag = _LaggedLog()
        zero = torch.zeros((), device=self.device)

        def emit(rec):
            if rec is not None and logf is not None:
                logf.write(json.dumps(rec) + "\n")
                logf.flush()
            return rec

        for _ in range(cfg.training.num_epochs):
            if isinstance(self.train_dataloader.sampler, torch.utils.data.distributed.DistributedSampler):
                self.train_dataloader.sampler.set_epoch(self.epoch)
            losses = []
            n_batches = len(self.train_dataloader)
            # H2D of the next batches on a copy stream from pinned staging, overlapped with the step
            for batch_idx, batch in enumerate(PinnedPrefetcher(self.train_dataloader, self.device)):
                if self.device_augment:
                    batch = augment_batch(batch)
                raw, lv, la = self.train_step(batch)
                meta = {"global_step": self.global_step, "epoch": self.epoch,
                        "lr": self.lr_scheduler.get_last_lr()[0]}
                grec = self.optimizer.grad_record if self.grad_guard_on() else None
                rec = emit(lag.push([raw, lv if lv is not None else zero, la if la is not None else zero], meta,
                                    record=grec, decode=self._grad_log if grec is not None else None))
                if rec is not None:
                    losses.append(rec["train_loss"])
                if batch_idx != n_batches - 1:
                    self.global_step += 1
                if cfg.training.max_train_steps is not None and batch_idx >= cfg.training.max_train_steps - 1:
                    break
            rec = emit(lag.flush())
            if rec is not None:
                losses.append(rec["train_loss"])
            step_log = {"train_loss": float(np.mean(losses)) if losses else float("nan"),
                        "global_step": self.global_step, "epoch": self.epoch}
            step_log.update(self.evaluate_epoch())
            if self.epoch % cfg.training.checkpoint_every == 0 and self.rank == 0:
                if cfg.checkpoint.save_last_ckpt:
                    self.save_checkpoint()
                metric = {k.replace("/", "_"): v for k, v in step_log.items()}
                path = topk.get_ckpt_path(metric)
                if path is not None:
                    self.save_checkpoint(path=path)
            emit(dict(step_log, epoch_end=True))
            self.global_step += 1
            self.epoch += 1
        self.wait_for_save()
        if logf is not None:
            logf.close()
        return self


def _precision(cfg):
    mp = str(cfg.training.get("mixed_precision", "fp16") or "no").lower()
    return "fp32" if mp in ("no", "fp32", "none") else "bf16"


def _broadcast_module_state(module, device):
    """rank 0's tensors of `module` to every rank (replaces the reference's normalizer pickle)."""
    sd = module.state_dict()
    keys = sorted(sd)
    meta = [(k, tuple(sd[k].shape)) for k in keys] if dist.get_rank() == 0 else None
    obj = [meta]
    dist.broadcast_object_list(obj, src=0)
    meta = obj[0]
    backend_dev = device if dist.get_backend() == "nccl" else torch.device("cpu")
    new = {}
    for k, shp in meta:
        t = sd[k].to(backend_dev).float().contiguous() if k in sd else torch.zeros(shp, device=backend_dev)
        dist.broadcast(t, src=0)
        new[k] = t.cpu()
    module.load_state_dict(new)
