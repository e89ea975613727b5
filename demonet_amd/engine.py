"""The loop around the hot path: the reference's `evaluate` (demonet/engine.py:70-110) with the forwards kept in flight.

The reference walks the data loader one batch at a time: images to the device, synchronize, `model(images)`, every output to the
host, `{image_id: output}` into the evaluator (engine.py:84-100). Here the same loop submits each batch to a
`pipeline.ForwardPipeline` and collects a batch's detections `depth` submissions later, so the device works on the next batches
while the host converts the previous ones: same `{image_id: {"boxes", "scores", "labels"}}` records (host tensors), same order.
The COCO evaluator itself (pycocotools, `data/coco_eval.py`) is third-party and absent here; `evalrec.coco_detection_records`
turns the records into the list `CocoEvaluator.prepare_for_coco_detection` builds (data/coco_eval.py:76-98) and
`evalrec.voc_mean_ap` scores them the PASCAL VOC way. `evaluate_voc` is the same loop with the scoring on the device: the detections stay
there and only the mAP comes back (demonet_amd/voceval.py). `evaluate_coco` is that loop with pycocotools' matching and its twelve numbers
(demonet_amd/cocoeval.py).

`train_one_epoch` is the reference's training loop (demonet/engine.py:14-56) for head fine-tuning: with `optim.SGD` the finiteness check of the
loss runs inside the optimizer's launch and the host reads the device once every `print_freq` steps.
"""
import collections
import functools
import math
import time
from typing import Dict, Iterable, List, Tuple

import torch

from .pipeline import ForwardPipeline


def _image_id(target):
    v = target["image_id"]
    return int(v.item()) if hasattr(v, "item") else int(v)


@torch.no_grad()
def evaluate(model, data_loader: Iterable, device="cuda:0", depth: int = 3) -> Tuple[Dict[int, Dict[str, torch.Tensor]], Dict[str, float]]:
    """data_loader yields (images, targets) as the reference's loaders do (engine.py:84): images = a list of [3,H,W] float tensors
    in [0,1] (or one [N,3,H,W] tensor), targets = a list of dicts holding "image_id". Batches whose images share one size go through
    the pipeline (any size: the device resizes to the network size and maps the boxes back, transform.py:27-53,278-292); a batch of
    mixed sizes is run by `model(images)` after the pipeline has drained, so the records keep the loader's order.
    Returns ({image_id: {"boxes" [n,4], "scores" [n], "labels" [n] int64}} on the host, {"images", "seconds", "images_per_sec",
    "model_seconds" (host time spent submitting and collecting)})."""
    device = torch.device(device)
    model.eval()
    results: Dict[int, Dict[str, torch.Tensor]] = collections.OrderedDict()
    pending = collections.deque()
    pipe = None
    shape = None
    n_images = 0
    model_time = 0.0

    def collect(ticket, ids):
        boxes, scores, labels, counts = pipe.result(ticket)
        host = [t.cpu() for t in (boxes, scores, labels, counts)]           # engine.py:92: outputs to the host
        for i, image_id in enumerate(ids):
            c = int(host[3][i])
            results[image_id] = {"boxes": host[0][i, :c].clone(), "scores": host[1][i, :c].clone(), "labels": host[2][i, :c].clone()}

    def drain():
        while pending:
            collect(*pending.popleft())

    t_start = time.perf_counter()
    for images, targets in data_loader:
        ids = [_image_id(t) for t in targets]
        same = isinstance(images, torch.Tensor) or len({tuple(im.shape) for im in images}) == 1
        t0 = time.perf_counter()
        if same:
            batch = images if isinstance(images, torch.Tensor) else torch.stack(list(images))
            batch = batch.to(device, non_blocking=True)
            if pipe is None or tuple(batch.shape) != shape:
                drain()
                if pipe is not None:
                    pipe.close()
                shape = tuple(batch.shape)
                pipe = ForwardPipeline(model, shape[0], height=shape[2], width=shape[3], depth=depth, device=device)
            if len(pending) == depth:                                       # its slot is about to be reused
                collect(*pending.popleft())
            pending.append((pipe.submit(batch), ids))
        else:
            drain()
            outputs = model([im.to(device) for im in images])              # engine.py:90
            for image_id, out in zip(ids, outputs):
                results[image_id] = {k: v.cpu() for k, v in out.items()}
        model_time += time.perf_counter() - t0
        n_images += len(ids)
    t0 = time.perf_counter()
    drain()
    if pipe is not None:
        pipe.close()
    model_time += time.perf_counter() - t0
    dt = time.perf_counter() - t_start
    return results, {"images": n_images, "seconds": dt, "images_per_sec": n_images / max(dt, 1e-9), "model_seconds": model_time}


def _evaluate_on_device(model, data_loader: Iterable, device, depth: int, acc) -> Tuple[int, float]:
    """`evaluate`'s loop with the detections left on the device: every batch goes to `acc.update(boxes, scores, labels, counts, targets)` on the
    current stream once its slot is about to be reused (`pipe.wait`: the current stream waits, the host does not), on the slot's own output
    tensors (`pipe.outputs`); the next submit on that slot orders itself behind the current stream. A batch of mixed sizes is run by
    `model(images)` after the pipeline has drained and padded to [n][detections_per_img]. Returns (images, model_seconds)."""
    model.eval()
    pending = collections.deque()
    pipe = None
    shape = None
    n_images = 0
    model_time = 0.0

    def collect(ticket, targets):
        pipe.wait(ticket)                                                   # the current stream waits; the host does not
        acc.update(*pipe.outputs(ticket), targets)

    def drain():
        while pending:
            collect(*pending.popleft())

    for images, targets in data_loader:
        same = isinstance(images, torch.Tensor) or len({tuple(im.shape) for im in images}) == 1
        t0 = time.perf_counter()
        if same:
            batch = images if isinstance(images, torch.Tensor) else torch.stack(list(images))
            batch = batch.to(device, non_blocking=True)
            if pipe is None or tuple(batch.shape) != shape:
                drain()
                if pipe is not None:
                    pipe.close()
                shape = tuple(batch.shape)
                pipe = ForwardPipeline(model, shape[0], height=shape[2], width=shape[3], depth=depth, device=device)
            if len(pending) == depth:                                       # its slot is about to be reused
                collect(*pending.popleft())
            pending.append((pipe.submit(batch), targets))
        else:
            drain()
            outputs = model([im.to(device) for im in images])
            n, D = len(outputs), model.detections_per_img
            boxes = torch.zeros((n, D, 4), dtype=torch.float32, device=device)
            scores = torch.zeros((n, D), dtype=torch.float32, device=device)
            labels = torch.zeros((n, D), dtype=torch.int64, device=device)
            lens = [int(o["scores"].shape[0]) for o in outputs]
            for i, (o, c) in enumerate(zip(outputs, lens)):
                boxes[i, :c], scores[i, :c], labels[i, :c] = o["boxes"], o["scores"], o["labels"]
            acc.update(boxes, scores, labels, torch.tensor(lens, dtype=torch.int32).to(device), targets)
        model_time += time.perf_counter() - t0
        n_images += len(targets)
    t0 = time.perf_counter()
    drain()
    if pipe is not None:
        pipe.close()
    model_time += time.perf_counter() - t0
    return n_images, model_time


@torch.no_grad()
def evaluate_voc(model, data_loader: Iterable, device="cuda:0", depth: int = 3, thresholds=(0.5,), use_07_metric: bool = False,
                 pixel_offset: float = 1.0) -> Tuple[dict, Dict[str, float]]:
    """PASCAL VOC mAP of `model` over `data_loader` with the detections left on the device. The loop is `evaluate`'s; the targets
    hold the reference's `boxes` [k, 4] xyxy, `labels` [k] and, optionally, `difficult` [k] (num_classes is the model's). A batch's detections
    never reach the host: once its slot is about to be reused, the current stream waits for the forward (`pipe.wait`) and
    `voceval.VocAccumulator.update` marks true and false positives there, on the slot's own output tensors (`pipe.outputs`), and keeps copies
    of scores, labels and flags on the device; the next submit on that slot orders itself behind the current stream. A batch of mixed sizes
    is run by `model(images)` after the pipeline has drained and padded to [n][detections_per_img]. Only `summarize` waits for the device.
    Returns (VocAccumulator.summarize(use_07_metric), stats) with the stats keys of `evaluate`; "seconds" includes the summary."""
    from .voceval import VocAccumulator
    device = torch.device(device)
    acc = VocAccumulator(model.graph.num_classes, thresholds, pixel_offset)
    t_start = time.perf_counter()
    n_images, model_time = _evaluate_on_device(model, data_loader, device, depth, acc)
    summary = acc.summarize(use_07_metric)
    dt = time.perf_counter() - t_start
    return summary, {"images": n_images, "seconds": dt, "images_per_sec": n_images / max(dt, 1e-9), "model_seconds": model_time}


@torch.no_grad()
def evaluate_coco(model, data_loader: Iterable, device="cuda:0", depth: int = 3, iou_thresholds=None, area_ranges=None,
                  max_dets=(1, 10, 100)) -> Tuple[dict, Dict[str, float]]:
    """The COCO numbers of `model` over `data_loader` with the detections left on the device: what the reference's `evaluate` gets
    from `CocoEvaluator` (data/coco_eval.py:23-64) and pycocotools. The loop is `evaluate_voc`'s; the targets hold the reference's `boxes`
    [k, 4] xyxy, `labels` [k] and, optionally, `iscrowd` [k] and `area` [k] (num_classes is the model's; the loader's order stands in for
    ascending image ids). `cocoeval.CocoAccumulator.update` matches every batch on the device and keeps scores, labels, flags and ranks
    there; only `summarize` waits for the device. Returns (CocoAccumulator.summarize() = {"stats": the twelve numbers, "precision", "recall"},
    stats) with the stats keys of `evaluate`; "seconds" includes the summary, "summarize_seconds" is the summary alone."""
    from . import cocoeval
    device = torch.device(device)
    acc = cocoeval.CocoAccumulator(model.graph.num_classes, cocoeval.IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds,
                                   cocoeval.AREA_RANGES if area_ranges is None else area_ranges, max_dets)
    t_start = time.perf_counter()
    n_images, model_time = _evaluate_on_device(model, data_loader, device, depth, acc)
    t0 = time.perf_counter()
    summary = acc.summarize()
    t1 = time.perf_counter()
    dt = t1 - t_start
    return summary, {"images": n_images, "seconds": dt, "images_per_sec": n_images / max(dt, 1e-9), "model_seconds": model_time,
                     "summarize_seconds": t1 - t0}


def _warmup(optimizer, n_batches: int):
    """The LR ramp of epoch 0: the rate climbs linearly from 1/1000 of its value to the whole of it over w = min(1000, n_batches - 1) scheduler
    steps and stays there (the reference's factor 1e-3 (1 - x/w) + x/w, engine.py:21-25, in its affine form)."""
    w = min(1000, n_batches - 1)
    return torch.optim.lr_scheduler.LambdaLR(optimizer, lambda x: 1.0 if x >= w else 1e-3 + (1.0 - 1e-3) * x / w)


class TrainLog:
    """What train_one_epoch returns: meters[name] = the list of per-step floats ("loss", every loss term, "lr" and, when the optimizer computes
    it, "grad_norm"); global_avg = {name: mean over the steps}."""

    def __init__(self):
        self.meters: Dict[str, List[float]] = collections.OrderedDict()

    def update(self, **values):
        for k, v in values.items():
            self.meters.setdefault(k, []).append(float(v))

    @property
    def global_avg(self) -> Dict[str, float]:
        return {k: sum(v) / len(v) for k, v in self.meters.items() if v}

    def line(self, names=None) -> str:
        """the last value and the mean of every meter, for a progress line"""
        return "  ".join("{}: {:.4g} ({:.4g})".format(k, v[-1], sum(v) / len(v)) for k, v in self.meters.items() if v and (names is None or k in names))

    def __str__(self):
        return self.line()


def train_one_epoch(model, optimizer, data_loader, device, epoch, print_freq, preset=None, generator=None) -> TrainLog:
    """The reference's train_one_epoch (engine.py:14-56): model.train(); on epoch 0 a linear LR warm-up from 1/1000 over
    min(1000, len(data_loader) - 1) iterations; per batch the loss dict of `model(images, targets)`, its sum, zero_grad, backward, optimizer step,
    scheduler step. data_loader yields (images, targets) and has a length. preset (e.g. model.train_preset()): images, targets =
    preset(images, targets, generator) first -- decoded uint8 images of any sizes to the network's input; without it the images are moved to
    `device` as they are, the targets' tensors with them. Returns a TrainLog; its "lr" is the rate each step used (the reference logs the rate
    after the scheduler's step, i.e. the next step's).

    With a demonet_amd.optim.SGD the loop does not wait for the device between log points: the loss terms gate the optimizer's launch (a step whose
    loss is not finite, and every step after it, writes nothing), every step's loss terms, their sum and the gradient norm go into a ring on the
    device, and the ring and the gate are read once every print_freq steps and once at the end. A tripped gate then raises FloatingPointError
    naming the step and its loss terms; parameters and momentum buffers are as of the last good step. The reference stops AT the first bad step
    (engine.py:41-44); this loop notices within print_freq steps, having changed nothing in between.
    With any other optimizer the loss is checked on the host every step, as the reference does (FloatingPointError instead of sys.exit)."""
    from .optim import SGD
    device = torch.device(device)
    print_freq = max(int(print_freq), 1)
    model.train()
    log = TrainLog()
    n_batches = len(data_loader)
    tag = f"epoch {epoch}"
    ramp = _warmup(optimizer, n_batches) if epoch == 0 else None
    ours = isinstance(optimizer, SGD)
    ring = None             # [print_freq][2 + terms] fp32 on the device: grad norm, loss terms, sum
    names: List[str] = []
    window: List[Tuple[int, float]] = []       # (iteration, lr) of the steps in the ring
    first_opt_step = optimizer.steps if ours else 0

    def read(i_last):
        host = ring[:len(window)].cpu()
        tripped, at = optimizer.status()
        bad = at - first_opt_step if tripped else None          # the iteration of the step that tripped the gate
        for row, (it, lr) in zip(host.tolist(), window):
            if bad is not None and it >= bad:
                if it == bad:
                    raise FloatingPointError("Loss is {} at step {} of epoch {}, stopping training: {} (parameters and momentum are those of step {})".format(
                        row[-1], it, epoch, dict(zip(names, row[1:-1])), it - 1))
                break
            log.update(loss=row[-1], **dict(zip(names, row[1:-1])))
            log.update(lr=lr)
            if optimizer.grad_norm is not None:
                log.update(grad_norm=row[0])
        if bad is not None:      # tripped by a step of an earlier window or of another caller
            raise FloatingPointError("the optimizer's gate tripped at its step {}, before iteration {} of epoch {}".format(at, window[0][0], epoch))
        window.clear()
        print(f"{tag}  step {i_last + 1}/{n_batches}  {log.line()}", flush=True)

    for i, (images, targets) in enumerate(data_loader):
        if preset is not None:
            images, targets = preset([image.to(device) for image in images], targets, generator)
        else:
            images = [im.to(device) for im in images]
            targets = [{k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in t.items()} for t in targets]
        loss_dict = model(images, targets)
        terms = list(loss_dict.values())
        losses = functools.reduce(torch.add, terms)
        if ours:
            if ring is None:
                names = list(loss_dict)
                ring = torch.zeros((print_freq, 2 + len(names)), dtype=torch.float32, device=losses.device)
            row = ring[len(window)]
            torch.stack([v.detach() for v in terms] + [losses.detach()], out=row[1:])
            optimizer.zero_grad()
            losses.backward()
            optimizer.step(gate=row[1:], norm_out=row[0:1])
            window.append((i, optimizer.param_groups[0]["lr"]))
        else:
            loss_value = losses.item()
            if not math.isfinite(loss_value):
                raise FloatingPointError("Loss is {} at step {} of epoch {}, stopping training: {}".format(
                    loss_value, i, epoch, {k: v.item() for k, v in loss_dict.items()}))
            optimizer.zero_grad()
            losses.backward()
            optimizer.step()
            log.update(loss=loss_value, **{k: v.item() for k, v in loss_dict.items()})
            log.update(lr=optimizer.param_groups[0]["lr"])
            if (i + 1) % print_freq == 0 or i + 1 == n_batches:
                print(f"{tag}  step {i + 1}/{n_batches}  {log.line()}", flush=True)
        if ramp is not None:
            ramp.step()
        if ours and len(window) == print_freq:
            read(i)
    if ours and window:
        read(n_batches - 1)
    return log


def coco_records(results: Dict[int, Dict[str, torch.Tensor]]) -> List[dict]:
    """The list `CocoEvaluator.prepare_for_coco_detection` builds from such a dict (data/coco_eval.py:76-98; xyxy -> xywh :162-164)."""
    out = []
    for image_id, pred in results.items():
        if len(pred["boxes"]) == 0:                                         # coco_eval.py:79-80
            continue
        b = pred["boxes"]
        xywh = torch.stack((b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), dim=1).tolist()
        scores, labels = pred["scores"].tolist(), pred["labels"].tolist()
        out.extend({"image_id": image_id, "category_id": labels[k], "bbox": xywh[k], "score": scores[k]} for k in range(len(xywh)))
    return out
