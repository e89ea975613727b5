"""Every kernel launch of the real plans against an fp32 error bound (oracle/op_ref.py).

Per configuration (model, classes, batch n, knobs set around plan creation and the forwards):
  labels    each op's kernel label from dn_profile_op_info after one profiled forward_batch (a separate model instance)
  parity    a DN_WS_REUSE=0 plan (every tensor keeps its own block): the whole span of tensor blocks and both head arrays are filled
            with 0xFF, then one dn_forward_heads. Every tensor block must be untouched (it stays inside a fused launch) or fully
            written, the gap bytes between blocks untouched, the head arrays fully written. Every op is then evaluated from the
            device's own values of the inputs it wrote (op_ref values of those it did not) and |got - y| <= E must hold for every
            element of every written tensor and of both head arrays.
  carry     the head outputs equal, bit for bit, those of the default plan (workspace reuse on) for the same model, images and n.
"""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest
import torch

import op_ref
from demonet_amd import _lib, models, synth

pytestmark = pytest.mark.gpu

V3, V2 = "ssdlite320_mobilenet_v3_large", "ssd_lite_mobilenet_v2"
CONFIGS = ([(V3, 91, n, {}, None) for n in (2, 16, 37, 64)]
           + [(V3, 91, 16, {k: v}, None) for k, v in (("DN_EXPDW", "0"), ("DN_TAIL", "0"), ("DN_HEAD_FUSE", "0"),
                                                      ("DN_SE_IN_DW", "1"), ("DN_PW_DW", "2"))]
           + [(V3, 91, 37, {"DN_XCD": "0"}, None), (V2, 21, 33, {}, None), (V2, 21, 16, {}, 300),
              ("ssd300_vgg16", 91, 5, {}, None), ("ssd300_vgg16", 91, 9, {}, None), ("ssd512_vgg16", 91, 3, {}, None),
              # the signature records conv_halo_kernel<3,8,2,head> (ssd300) and pw_kernel<64,64,2,2,true,32> (ssd512) at n = 16 only
              ("ssd300_vgg16", 91, 16, {}, None), ("ssd512_vgg16", 91, 16, {}, None)])
# The V2 plan at other network sizes: every decision of the planner and the choice functions that depends on a map size takes one branch
# at 300 / 320. 160: level 1 is 5 x 5 (under the 32 pixels of the softmax epilogue), the 160- / 320-channel blocks and the 1280-channel 1x1
# become tail-eligible; 192: level 1 is 6 x 6; 224: 7 -> 4 -> 2 -> 1 -> 1; 301: an odd input, a stem column without a right neighbour;
# 496 / 512: level 0 is 31 / 32 wide, the last width the fused head launch takes and the first it does not; 640: 40 x 40, the last level
# 2 x 2. 9 images: XCD grouping with ragged groups.
V2_SIZES = (160, 192, 224, 256, 301, 384, 496, 512, 640)
SIZE_CONFIGS = ([(V2, 21, 2 if size == 640 else 3, {}, size) for size in V2_SIZES]
                + [(V2, 21, 9, {}, size) for size in (160, 301, 496)]
                + [(V2, 21, 3, {k: "0"}, size) for size in (160, 512) for k in ("DN_TAIL", "DN_HEAD_FUSE")])
CONFIGS = CONFIGS + SIZE_CONFIGS


def _cid(c):
    name, ncls, n, env, size = c
    return "-".join([name, f"n{n}"] + [f"{k}={v}" for k, v in env.items()] + ([f"size{size}"] if size else []))


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _model(name, ncls, size, dev, weights=None):
    """weights: None for the synthetic weights, or a regime of tests/trained_like.py"""
    m = getattr(models, name)(num_classes=ncls, **({"image_size": size} if size else {}))
    if weights is not None:
        import trained_like
        return trained_like.load(m, weights).to(dev)
    return models.load_synthetic(m, 0).to(dev)


def _labels(m, imgs, dev):
    """per op: the label of the launch it took part in and the op that owns that launch's time segment (dn_profile_op_info after one
    profiled forward_batch)"""
    L = _lib.lib()
    h = C.c_void_p(m._plan(dev))
    _lib.check(L.dn_profile_begin(h))
    m.forward_batch(imgs, persistent_input=True)
    nseg = len(m.graph.nodes) + 4
    _lib.check(L.dn_profile_end(h, (C.c_float * nseg)(), nseg))
    label, owner = C.create_string_buffer(96), C.c_int32()
    out, owners = [], []
    for i in range(len(m.graph.nodes)):
        _lib.check(L.dn_profile_op_info(h, i, label, 96, C.byref(owner)))
        # forward_heads never runs the softmax epilogue of the fused head launch (dn_forward does, from 32 images per chain): the
        # instantiation checked here is the plain one
        out.append(label.value.decode().replace(",softmax", ""))
        owners.append(int(owner.value))
    return out, owners


class _Stats:
    def __init__(self):
        self.count, self.worst, self.where = {}, {}, {}

    def add(self, label, n, ratio, where):
        self.count[label] = self.count.get(label, 0) + n
        if ratio >= self.worst.get(label, -1.0):
            self.worst[label], self.where[label] = ratio, where


def _check(what, label, got, y, e, fp16, stats, fails, layout="nchw"):
    """|got - y| <= E (+ 0.5 ulp16(|got|) for fp16 storage) for every element; records count and worst ratio per label"""
    r = op_ref.ratio(got, y, e, fp16)
    bad = ~(r <= 1.0)                   # (NaN fails)
    k = int(torch.argmax(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)))
    idx = np.unravel_index(k, tuple(r.shape))
    ratio = float(r.reshape(-1)[k])
    where = f"{what} [{label}] worst at {layout} {tuple(int(v) for v in idx)}: got {float(got.reshape(-1)[k]):.6g} y {float(y.reshape(-1)[k]):.6g} " \
            f"ratio {ratio:.3f}"
    stats.add(label, r.numel(), ratio, where)
    if bool(bad.any()):
        fails.append(f"{where} ({int(bad.sum())} of {r.numel()} elements over the bound)")


_CACHE = {}


def _run(cfg, weights=None):
    name, ncls, n, env, size = cfg
    key = _cid(cfg) + f"-K{ncls}" + (f"-{weights}" if weights else "")         # (the test ids leave the class count out; the results must not)
    if key in _CACHE:
        return _CACHE[key]
    dev = torch.device("cuda:0")
    L = _lib.lib()
    t0 = time.time()
    with _Env(env):
        lab_m = _model(name, ncls, size, dev, weights)
        g = lab_m.graph
        W, H = g.size
        imgs = torch.from_numpy(synth.images(11, n, H, W))
        imgs_d = imgs.to(dev)
        labels, owners = _labels(lab_m, imgs_d, dev)
        ref_logits, ref_reg = lab_m.forward_heads(imgs_d)            # the default plan (workspace reuse as configured by default)
        torch.cuda.synchronize()
        lab_m.release()
        with _Env({"DN_WS_REUSE": "0"}):
            m = _model(name, ncls, size, dev, weights)
            h = C.c_void_p(m._plan(dev))
            b = m._buffers_for(n, H, W, dev)
            ws = b["ws"]
            base = ws.data_ptr()
            pl, pr = C.c_void_p(), C.c_void_p()
            _lib.check(L.dn_head_outputs(h, C.c_void_p(base), n, C.byref(pl), C.byref(pr)))     # before the plan's first forward
            A, K = g.num_anchors(), g.num_classes
            lo, ro = pl.value - base, pr.value - base
            blocks = {}
            ptr, sz = C.c_void_p(), C.c_size_t()
            for tid, t in enumerate(g.tensors):
                if t.kind == "image":
                    continue
                _lib.check(L.dn_tensor_ptr(h, C.c_void_p(base), n, tid, C.byref(ptr), C.byref(sz)))
                blocks[tid] = (ptr.value - base, sz.value)
            spans = sorted(blocks.values())
            end = (max(o + s for o, s in spans) + 255) // 256 * 256         # (blocks are 256-byte aligned: the last one's pad too)
            assert end <= min(lo, ro), "tensor blocks overlap the head arrays"
            ws[:end].fill_(255)
            ws[lo:lo + n * A * K * 4].fill_(255)
            ws[ro:ro + n * A * 16].fill_(255)
            logits, reg = m.forward_heads(imgs_d)
            torch.cuda.synchronize()
    fails, stats = [], _Stats()
    # coverage: gap bytes untouched, every block untouched or fully written, head arrays fully written
    at = 0
    for o, s in spans + [(end, 0)]:
        if o > at and not bool((ws[at:o] == 255).all()):
            fails.append(f"bytes [{at}, {o}) between tensor blocks were written")
        at = max(at, o + s)
    written = {}
    for tid, (o, s) in blocks.items():
        t = g.t(tid)
        v = ws[o:o + s].view(torch.int16 if t.kind == "act" else torch.int32)
        untouched = int((v == -1).sum())
        if untouched == v.numel():
            written[tid] = False
        elif untouched == 0:
            written[tid] = True
        else:
            fails.append(f"tensor {tid} ({t.kind} {t.c}x{t.h}x{t.w}) partly written: {untouched} of {v.numel()} elements untouched")
            written[tid] = True
    for what, arr in (("cls_logits", logits), ("bbox_regression", reg)):
        u = int((arr.view(torch.int32) == -1).sum())
        if u:
            fails.append(f"head array {what}: {u} of {arr.numel()} elements not written")
    if fails:
        m.release()
        return _CACHE.setdefault(key, dict(labels=labels, owners=owners, graph=g, stats=stats, fails=fails, seconds=time.time() - t0))
    # carry-over to the default plan
    if not (torch.equal(logits, ref_logits) and torch.equal(reg, ref_reg)):
        fails.append(f"head outputs of the DN_WS_REUSE=0 plan differ from the default plan's: "
                     f"max|d| {(logits - ref_logits).abs().max().item():.3g} / {(reg - ref_reg).abs().max().item():.3g}")

    def device(tid):
        o, s = blocks[tid]
        t = g.t(tid)
        if t.kind == "act":
            return ws[o:o + s].view(torch.float16).view(n, t.h, t.w, t.c).float().cpu().permute(0, 3, 1, 2).contiguous()
        if t.kind == "vec":
            return ws[o:o + s].view(torch.float32).view(n, t.c).cpu()
        return ws[o:o + s].view(torch.float32).view(n, -1, t.c).double().sum(1).float().cpu()      # pool partials: sum over tiles

    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items() if v.is_floating_point()}
    ref = op_ref.OpRef(g, sd)
    last = {}
    for i, nd in enumerate(g.nodes):
        for tid in (nd.inp, nd.residual, nd.se):
            if tid >= 0:
                last[tid] = i
    lvl_off = np.cumsum([0] + [a * g.t(f).h * g.t(f).w for a, f in zip(g.anchors_per_loc, g.features)])
    val, err = {g.nodes[0].inp: op_ref.stem_input(g, imgs)}, {}
    head_arr = {1: logits.cpu(), 2: reg.cpu()}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with torch.no_grad():
        for i, nd in enumerate(g.nodes):
            y, e = ref.op(nd, val, err)
            lab = labels[i]
            what = f"op {i} {nd.op} {nd.conv_key or nd.fc1_key or nd.scale_key} -> t{nd.out}"
            if nd.head and nd.op in ("pw", "conv"):
                rows = slice(int(lvl_off[nd.level]), int(lvl_off[nd.level + 1]))
                got = head_arr[nd.head][:, rows]
                _check(what, lab, got, op_ref.head_rows(g, nd, y), op_ref.head_rows(g, nd, e), False, stats, fails, "(image, anchor row, col)")
            elif nd.op == "se":
                if written[nd.out]:
                    got = device(nd.out)
                    _check(what, lab, got, y, e, False, stats, fails, "(image, channel)")
                    val[nd.out], err[nd.out] = got, None
                else:
                    val[nd.out], err[nd.out] = y, e
            else:
                if nd.op == "dw" and nd.pool >= 0:
                    s, es = op_ref.pool_sum(y, e)
                    if written[nd.pool]:
                        got = device(nd.pool)
                        _check(what + " pooled sums", lab, got, s, es, False, stats, fails, "(image, channel)")
                        val[nd.pool], err[nd.pool] = got, None
                    else:
                        val[nd.pool], err[nd.pool] = s, es
                if written[nd.out]:
                    got = device(nd.out)
                    _check(what, lab, got, y, e, True, stats, fails, "(image, channel, y, x)")
                    val[nd.out], err[nd.out] = got, None
                else:
                    val[nd.out], err[nd.out] = op_ref.entered(y, e)
            for tid in (nd.inp, nd.residual, nd.se):
                if tid >= 0 and last.get(tid) == i:
                    val.pop(tid, None)
                    err.pop(tid, None)
    m.release()
    return _CACHE.setdefault(key, dict(labels=labels, owners=owners, graph=g, stats=stats, fails=fails, seconds=time.time() - t0))


def _report(res, title):
    lines = [f"{title}  ({res['seconds']:.1f} s)"]
    st = res["stats"]
    for lab in sorted(st.count):
        lines.append(f"  {lab:44s} {st.count[lab]:>12d} elements   max |got - y| / E {st.worst[lab]:.3f}")
    return "\n".join(lines)


@pytest.mark.parametrize("cfg", CONFIGS, ids=[_cid(c) for c in CONFIGS])
def test_launch_parity(cfg):
    res = _run(cfg)
    print("\n" + _report(res, _cid(cfg)))
    assert not res["fails"], "\n".join(res["fails"][:20])


def _tail_op_supported(g, nd):
    """tail.hip tail_op_supported on a graph node (the fragment-major weight copy every 1x1 of these graphs has is taken for granted)"""
    ti, to = g.t(nd.inp), g.t(nd.out)
    if nd.head or nd.residual >= 0 or nd.se >= 0 or nd.pool >= 0:
        return False
    if nd.op == "pw":
        return to.h * to.w <= 32 and nd.cin % 16 == 0 and nd.cout % 8 == 0 and nd.cin <= 2048 and nd.cout <= 2048
    if nd.op == "dw":
        return to.h * to.w <= 32 and ti.h * ti.w <= 128 and nd.cin % 8 == 0 and nd.dil == 1 and nd.k in (3, 5)
    return False


@pytest.mark.parametrize("cfg", SIZE_CONFIGS, ids=[_cid(c) for c in SIZE_CONFIGS])
def test_the_launches_are_the_ones_the_map_sizes_call_for(cfg):
    """Which path ran, from the graph's map sizes alone: a plan that quietly left everything on the per-op and grouped launches would pass the
    parity test. Fused head launch: the levels whose heads are depthwise -> 1x1 on a map of W <= 31 with C % 32 == 0 and ReLU6
    (headfuse.hip head_fused_level_supported; the V2 model's last level is a plain 1x1). Tail run: the longest linear suffix of the backbone
    whose ops pass tail_op_supported and are not part of an earlier multi-op launch, cut to TAIL_MAX_OPS = 16, at least two ops."""
    name, ncls, n, env, size = cfg
    res = _run(cfg)
    g, labels, owners = res["graph"], res["labels"], res["owners"]
    nodes = g.nodes
    producer = {nd.out: i for i, nd in enumerate(nodes)}
    # ---- the fused head launch
    want_levels = set()
    for i, nd in enumerate(nodes):
        if nd.head != 1 or nd.op != "pw":
            continue
        d = nodes[producer[nd.inp]] if nd.inp not in g.features else None
        t = g.t(g.features[nd.level])
        if d is not None and d.op == "dw" and t.w <= 31 and t.c % 32 == 0 and t.c >= 32 and d.act == 2 and env.get("DN_HEAD_FUSE", "1") != "0":
            want_levels.add(nd.level)
    got_levels = set()
    for i, nd in enumerate(nodes):
        if nd.head and nd.op == "pw":
            ops = [i] + ([producer[nd.inp]] if nd.inp not in g.features else [])
            fused = [labels[q].startswith("head_fused_kernel") for q in ops]
            assert all(fused) or not any(fused), f"level {nd.level}: {[labels[q] for q in ops]}"
            if fused[0]:
                got_levels.add(nd.level)
            else:
                assert nd.level not in want_levels, f"level {nd.level} ({g.t(g.features[nd.level]).w} wide) left the fused head launch: {labels[i]}"
    assert got_levels == want_levels, (sorted(got_levels), sorted(want_levels))
    widths = [g.t(f).w for f in g.features]
    assert want_levels == (set() if env.get("DN_HEAD_FUSE") == "0" else {l for l in range(5) if widths[l] <= 31}), (widths, want_levels)
    # ---- the tail run
    end = min(i for i, nd in enumerate(nodes) if nd.head or any(u.head and u.inp == nd.out and nd.out not in g.features for u in nodes))
    members = {}
    for i, o in enumerate(owners):
        members.setdefault(o, []).append(i)
    other_launch = lambda i: labels[i] != "tail_kernel" and len(members[owners[i]]) > 1       # grouped before the tail pass (expand -> depthwise -> project)
    first = end
    while first > 0:
        i = first - 1
        if other_launch(i) or not _tail_op_supported(g, nodes[i]) or (first < end and nodes[first].inp != nodes[i].out):
            break
        first -= 1
    first = max(first, end - 16)
    want_tail = set(range(first, end)) if end - first >= 2 and env.get("DN_TAIL", "1") != "0" else set()
    got_tail = {i for i, lab in enumerate(labels) if lab == "tail_kernel"}
    print(f"\n{_cid(cfg)}: fused head levels {sorted(got_levels)} of widths {widths}; tail run ops {min(got_tail, default=-1)} .. {max(got_tail, default=-1)} "
          f"({len(got_tail)} ops), backbone ends at {end}")
    assert got_tail == want_tail, (sorted(got_tail), sorted(want_tail))
    if env.get("DN_TAIL", "1") != "0":
        assert len(want_tail) >= 8, "every size has the extra layers' tiny maps in its tail run"


def test_parity_covers_every_signature_label(golden_dir):
    """the kernel labels checked above cover every label of tests/golden/plan_signature.json (the softmax instantiations of the fused head
    launch excepted: dn_forward runs them from 32 images per chain, and test_gpu_model.py holds them bit-identical to the plain ones)"""
    with open(os.path.join(golden_dir, "plan_signature.json")) as f:
        sig = json.load(f)
    want = {lab for cfg in sig.values() for row in cfg["ops"].values() for lab, _ in row if ",softmax" not in lab}
    seen, total = {}, _Stats()
    for cfg in CONFIGS:
        res = _run(cfg)
        for lab in res["stats"].count:
            seen.setdefault(lab, []).append(_cid(cfg))
            total.add(lab, res["stats"].count[lab], res["stats"].worst[lab], res["stats"].where[lab])
    print("\nall configurations: label, elements checked, worst |got - y| / E")
    for lab in sorted(total.count):
        print(f"  {lab:44s} {total.count[lab]:>13d}   {total.worst[lab]:.3f}")
    print("  total wall time of the configurations: %.1f s" % sum(_run(c)["seconds"] for c in CONFIGS))
    missing = sorted(want - set(seen))
    assert not missing, f"labels of the plan signature no configuration checks: {missing}"
