"""The head launches across class counts. K = num_classes is the factory argument every user sets; with 6 anchors per location the class head
of an SSDLite level has nc0 = 6 K channels, and from K follow
  the head_fused_kernel<TCW, SM> instantiation  ct0 = ceil(6 K / 32) class tiles + one box tile, TCW = ceil((ct0 + 1) / 4) in 1 .. 5;
  the wave that owns the box tile               tile index ct0, wave ct0 % 4 (tlast / last_reg / last_on in the kernel);
  whether the last class tile is ragged         6 K % 32;
  whether the fused launch is taken at all      TCW <= 5: K <= 101 (headfuse.hip head_fused_level_supported);
  the softmax / decode epilogue's row geometry  three batches of 32 classes over four lanes, K <= 92; the per-class bins by nb + K - 1 <= 256;
  the tile of the grouped launches              choice.h pw_group_choose: 128 x 32 up to 32 channels, 64 x 64 up to 64, then by fill.
Everything else in the suite holds a kernel to a reference at K = 21 and 91 (and above 256). Here: the per-launch parity of
tests/test_gpu_launch_parity.py (same machinery, same bound E of oracle/op_ref.py) at the K that flip those decisions, the labels held to a
restatement of the rules, the epilogue against the logit-writing path AND against the oracle's post-process, and the 101 / 102 boundary."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import ssd_oracle as so
import test_gpu_launch_parity as lp
from demonet_amd import _lib, models, synth

pytestmark = pytest.mark.gpu

V3, V2 = lp.V3, lp.V2
cdiv = lambda a, b: -(-a // b)


def _tiles(K, aloc=6):
    """(ct0, TCW, wave of the box tile, channels of the last class tile beyond a whole tile) of a level with `aloc` anchors per location"""
    ct0 = cdiv(aloc * K, 32)
    return ct0, cdiv(ct0 + 1, 4), ct0 % 4, (aloc * K) % 32


#   K: (6 K, ct0, TCW, box tile on wave, 6 K % 32)      why
TABLE = {2: (12, 1, 1, 1, 12),      # smallest K; waves 2 and 3 idle; group tile 128 x 32
         10: (60, 2, 1, 2, 28),     # group tile 64 x 64 (maxc <= 64)
         16: (96, 3, 1, 3, 0),      # all four waves busy, exact tiles
         32: (192, 6, 2, 2, 0),     # softmax batch edge
         33: (198, 7, 2, 3, 6),     # the other side of it
         48: (288, 9, 3, 1, 0),     # TCW 3
         58: (348, 11, 3, 3, 28),   # last K of TCW 3
         59: (354, 12, 4, 0, 2),    # first K of TCW 4
         65: (390, 13, 4, 1, 6),    # TCW 4, second batch edge
         80: (480, 15, 4, 3, 0),    # last K of TCW 4
         101: (606, 19, 5, 3, 30),  # last fused K
         102: (612, 20, 6, 0, 4)}   # TCW would be 6: the first K on the grouped launches

# (model, classes, images, knobs, network size): the configurations of test_gpu_launch_parity.py with the class count as the axis
CONFIGS = ([(V3, k, 2, {}, None) for k in TABLE]
           + [(V3, k, 9, {}, None) for k in (2, 58, 59)]                    # XCD grouping with ragged groups at TCW 1, 3, 4 (box tile on waves 1, 3, 0)
           + [(V3, k, 2, {"DN_HEAD_FUSE": "0"}, None) for k in (2, 10, 48)]      # the three maxc regimes of pw_group_choose
           + [(V2, 48, 3, {}, 160), (V2, 80, 3, {}, 160),
              (V2, 48, 3, {}, 512)])                                        # level 0 is outside the fused launch: a fused and a grouped head launch at one K
# (ssd300_vgg16 at K = 2 and 10 -- the dense-conv group tiles at maxc <= 32 and <= 64 -- passed when measured, at 2.4 s with two images and 1.9 s
#  with one against 1.1 - 1.25 s of the parity file's ssdlite320 n16 configuration, the time limit set for a case of this file: left out)


def _cid(c):
    return lp._cid(c) + f"-K{c[1]}"


IDS = [_cid(c) for c in CONFIGS]


def test_the_table_is_the_arithmetic_of_the_launcher():
    for K, (nc0, ct0, tcw, wave, rag) in TABLE.items():
        assert (6 * K,) + _tiles(K) == (nc0, ct0, tcw, wave, rag), K
    assert {v[2] for v in TABLE.values()} == {1, 2, 3, 4, 5, 6} and {v[3] for k, v in TABLE.items() if k <= 101} == {0, 1, 2, 3}
    assert _tiles(101)[1] == 5 and _tiles(102)[1] == 6


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_launch_parity_across_class_counts(cfg):
    res = lp._run(cfg)
    print("\n" + lp._report(res, _cid(cfg)))
    st = res["stats"]
    if st.worst:
        lab = max(st.worst, key=st.worst.get)
        print(f"  closest to the bound: {st.worst[lab]:.6f}  {st.where[lab]}")
        heads = {l: v for l, v in st.worst.items() if l.startswith(("head_fused_kernel", "pw_group_kernel"))}
        print("  head launches: " + ", ".join(f"{l} {v:.3f}" for l, v in sorted(heads.items())))
    assert not res["fails"], "\n".join(res["fails"][:20])
    assert sum(st.count.values()) > 0 and all(np.isfinite(v) for v in st.worst.values())


# ---- which launches K calls for ---------------------------------------------------------------------------------------------------
PW_FILL_WGS = 1500                # choice.h
GROUP_WAVES = {(128, 32): (4, 1), (64, 64): (2, 2), (128, 128): (2, 2), (128, 96): (4, 1), (64, 128): (2, 2)}      # pointwise.hip PW_GROUP_TILES: WP, WC of a tile


def _group_choose(problems):
    """choice.h pw_group_choose for 1x1 problems, on (rows m, output channels) pairs: the tile (bp, bc) and the launch's 128 x 128 workgroups"""
    maxc = max(c for _, c in problems)
    wg128 = sum(cdiv(m, 128) * cdiv(c, 128) for m, c in problems)
    if maxc <= 32:
        tile = (128, 32)
    elif maxc <= 64:
        tile = (64, 64)
    elif wg128 >= PW_FILL_WGS:
        narrow = sum(m * cdiv(c, 96) * 96 for m, c in problems) <= 0.95 * sum(m * cdiv(c, 128) * 128 for m, c in problems)
        tile = (128, 96) if narrow else (128, 128)
    else:
        tile = (64, 128)
    return tile, wg128


def _group_label(tile):
    wp, wc = GROUP_WAVES[tile]
    return f"pw_group_kernel<{tile[0]},{tile[1]},{wp},{wc},false,32,3>"       # (launch_group_tile's label: 32-deep stages requested 3 ahead)


def _expected_head_launches(g, n, env):
    """From the graph and K alone: the levels of the fused head launch and its TCW, and the label of the grouped 1x1 launch that takes the
    rest. head_fused_level_supported (headfuse.hip): depthwise 3x3 + ReLU6 -> 1x1 on a map of W <= 31 with C % 32 == 0, at most 32 box channels,
    even channel counts, ceil((ceil(nc0 / 32) + 1) / 4) <= 5 (the 2^31 / 2^32 limits of the function are far away at these sizes); plan.hip
    fused_head_levels: a level joins only with the first level's (ceil(nc0 / 32) + 4) / 4. run_head_groups: what is left leaves as ONE group launch
    (class and box heads together, at most 12 problems), its tile by pw_group_choose."""
    nodes = g.nodes
    producer = {nd.out: i for i, nd in enumerate(nodes)}
    cls = {nd.level: i for i, nd in enumerate(nodes) if nd.head == 1 and nd.op == "pw"}
    reg = {nd.level: i for i, nd in enumerate(nodes) if nd.head == 2 and nd.op == "pw"}
    assert sorted(cls) == sorted(reg) == list(range(len(g.features)))
    fused, first = [], None
    for lv in sorted(cls):
        c, r = nodes[cls[lv]], nodes[reg[lv]]
        t = g.t(g.features[lv])
        dws = [nodes[producer[x.inp]] if x.inp not in g.features else None for x in (c, r)]
        ok = (env.get("DN_HEAD_FUSE", "1") != "0" and all(d is not None and d.op == "dw" and d.k == 3 and d.act == 2 for d in dws)
              and t.w <= 31 and t.c % 32 == 0 and t.c >= 32 and r.cout <= 32 and c.cout % 2 == 0 and r.cout % 2 == 0 and cdiv(cdiv(c.cout, 32) + 1, 4) <= 5)
        if ok and first is not None and (cdiv(c.cout, 32) + 4) // 4 != (cdiv(first, 32) + 4) // 4:
            ok = False
        if ok:
            first = c.cout if first is None else first
            fused.append(lv)
    tcw = cdiv(cdiv(first, 32) + 1, 4) if fused else None
    rest = [lv for lv in sorted(cls) if lv not in fused]
    group = None
    if rest:
        problems = [(n * g.t(g.features[lv]).h * g.t(g.features[lv]).w, nodes[q[lv]].cout) for lv in rest for q in (reg, cls)]
        assert len(problems) <= 12
        tile, wg128 = _group_choose(problems)
        group = dict(levels=rest, tile=tile, label=_group_label(tile), wg128=wg128)
    return dict(fused=fused, tcw=tcw, group=group, cls=cls, reg=reg, producer=producer)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_the_launches_are_the_ones_the_class_count_calls_for(cfg):
    """A plan that quietly left the fused launch, or took another instantiation than the one K calls for, would pass the parity test."""
    name, ncls, n, env, size = cfg
    res = lp._run(cfg)
    g, labels = res["graph"], res["labels"]
    want = _expected_head_launches(g, n, env)
    # what the rules must give for these configurations, said outright
    widths = [g.t(f).w for f in g.features]
    if name == V3:
        assert want["fused"] == ([] if ncls >= 102 or env.get("DN_HEAD_FUSE") == "0" else list(range(6))), want["fused"]
    else:
        assert want["fused"] == [lv for lv in range(5) if widths[lv] <= 31], (widths, want["fused"])      # (the V2 model's last level is a plain 1x1)
    if want["fused"]:
        assert want["tcw"] == _tiles(ncls)[1] <= 5
    for lv in sorted(want["cls"]):
        ops = []
        for q in (want["cls"][lv], want["reg"][lv]):
            ops.append(q)
            if g.nodes[q].inp not in g.features:
                ops.append(want["producer"][g.nodes[q].inp])
        got = [labels[q] for q in ops]
        if lv in want["fused"]:
            assert got == [f"head_fused_kernel<{want['tcw']}>"] * len(ops), (lv, got)
        else:
            assert not any(l.startswith("head_fused_kernel") for l in got), (lv, got)
            assert labels[want["cls"][lv]] == labels[want["reg"][lv]] == want["group"]["label"], (lv, got, want["group"])
    print(f"\n{_cid(cfg)}: fused levels {want['fused']} as head_fused_kernel<{want['tcw']}>, grouped "
          f"{want['group'] and (want['group']['levels'], want['group']['label'], want['group']['wg128'])}")


def test_the_configurations_reach_every_instantiation_the_class_count_selects():
    """head_fused_kernel<T> for every T, and every tile pw_group_choose can return for the 1x1 heads of a 6-anchor model at these batches. The two
    tiles of the `wg128 >= PW_FILL_WGS` branch are NOT reached and are named here: 1500 workgroups of 128 x 128 take 59 images of the V3 model at
    K = 102 (25 workgroups per image) and more at any smaller K, and op_ref's fp32 evaluation of that many images is minutes of CPU time."""
    seen, wg_max = set(), 0
    for cfg in CONFIGS:
        res = lp._run(cfg)
        seen |= set(res["labels"])
        grp = _expected_head_launches(res["graph"], cfg[2], cfg[3])["group"]
        if grp:
            wg_max = max(wg_max, grp["wg128"])
    fused = sorted(l for l in seen if l.startswith("head_fused_kernel"))
    assert fused == [f"head_fused_kernel<{t}>" for t in (1, 2, 3, 4, 5)], fused
    reached = [_group_label(t) for t in ((128, 32), (64, 64), (64, 128))]
    not_reached = [_group_label(t) for t in ((128, 96), (128, 128))]
    for lab in reached:
        assert lab in seen, (lab, sorted(l for l in seen if l.startswith("pw_group_kernel")))
    assert wg_max < PW_FILL_WGS and not any(lab in seen for lab in not_reached), (wg_max, sorted(seen))
    print(f"\nfused: {fused}\ngrouped: {sorted(l for l in seen if l.startswith('pw_group_kernel'))}\nlargest 1x1 head group: {wg_max} workgroups of 128 x 128 "
          f"(the 128 x 96 / 128 x 128 tiles start at {PW_FILL_WGS})")


# ---- the softmax / decode epilogue across K -----------------------------------------------------------------------------------------
def _hist_nb(score_thresh):
    """postprocess.hip post_hist_range, the one function both plan.hip (head_softmax_epilogue -> HeadPost::nb) and launch_postprocess call: the
    histogram bins are float bits >> 19, the top bin is 1.0's, at most 256 are kept; nb = bins that a score in (score_thresh, 1] can reach"""
    bits = lambda f: struct.unpack("<I", struct.pack("<f", f))[0]
    top, hb_thr = bits(1.0) >> 19, bits(max(score_thresh, 0.0)) >> 19
    return top + 1 - max(hb_thr, top + 1 - 256)


def _risky(m):
    # a near-tie that 1-ulp softmax differences could flip (exact ties, gap 0, break canonically): the rule of test_num_classes_and_postprocess_kwargs
    return min(m["thresh_gap"], m["iou_gap"]) < 1e-5 or any(0 < m[k] < 1e-5 for k in ("topk_gap", "final_gap", "order_gap"))


# With the factories' thresholds (score_thresh 0.001, 300 candidates per class, 300 detections) every image has a near-tie somewhere among its
# 10^5 passing scores, and at small K the synthetic heads (|logit| up to 17) saturate the best scores to within a few ulp of 1: nothing but counts
# and sorted scores would ever be compared. So that labels and boxes ARE compared, a case keeps 10 detections above a score_thresh that about 60
# scores of an image pass (the 61st largest score of image seed 500, two decimals), and at K = 2, 5 and 16 the class heads' last 1x1 (weights and
# bias) is scaled by `cool`, which takes the logits out of saturation. The launch computes and stores every score of every class whatever the
# threshold. The two last cases put score_thresh on either side of the per-class bins' switch at K = 5 (nb = 253 / 252: nb + K - 1 = 257 / 256),
# where every score of the image passes and is counted, with 10 candidates per class.
# (model, K, network size, cool, post-process attributes, per-class bins on, image seeds). Seeds: picked on the CPU, the first five from 500 up for
# which ssd_oracle.selection_margins of the oracle's own post-process on the fp32 logits of the CPU path (OracleSSD.forward_raw) shows no margin
# below 1e-4 (thresh_gap, iou_gap; topk_gap, final_gap, order_gap where not exactly 0). Of the 113 images scanned 4 had a margin below the 1e-5 of
# the tests, all in final_gap.
EPILOGUE_CASES = [
    (V3, 2, None, 0.25, dict(detections_per_img=10, score_thresh=0.9), True, [500, 501, 507, 510, 511]),
    (V3, 5, None, 0.25, dict(detections_per_img=10, score_thresh=0.54), True, [501, 502, 503, 504, 505]),
    (V3, 16, None, 0.5, dict(detections_per_img=10, score_thresh=0.75), True, [500, 501, 502, 503, 504]),
    (V3, 32, None, 1.0, dict(detections_per_img=10, score_thresh=0.93), True, [501, 504, 505, 508, 509]),
    (V3, 33, None, 1.0, dict(detections_per_img=10, score_thresh=0.93), True, [501, 504, 505, 508, 510]),
    (V3, 48, None, 1.0, dict(detections_per_img=10, score_thresh=0.87), True, [501, 502, 503, 507, 511]),
    (V3, 64, None, 1.0, dict(detections_per_img=10, score_thresh=0.86), True, [500, 501, 503, 504, 506]),
    (V3, 65, None, 1.0, dict(detections_per_img=10, score_thresh=0.86), True, [500, 501, 502, 503, 504]),
    (V3, 80, None, 1.0, dict(detections_per_img=10, score_thresh=0.87), True, [502, 503, 504, 505, 507]),
    (V3, 92, None, 1.0, dict(detections_per_img=10, score_thresh=0.85), True, [500, 501, 502, 504, 506]),
    (V2, 48, 160, 1.0, dict(detections_per_img=10, score_thresh=0.88), True, [504, 505, 506, 512, 513]),
    (V3, 5, None, 0.25, dict(topk_candidates=10, detections_per_img=20, score_thresh=1.95e-5), False, [502, 503, 504, 505, 507]),
    (V3, 5, None, 0.25, dict(topk_candidates=10, detections_per_img=20, score_thresh=2.05e-5), True, [502, 503, 504, 505, 507]),
]


def _cooled_model(name, ncls, size, cool, post):
    """the synthetic weights with the class heads' last convolution scaled by `cool`, the post-process attributes set as on the reference's module;
    returns the model and the state dict it holds"""
    m = getattr(models, name)(num_classes=ncls, **({"image_size": size} if size else {}))
    sd = synth.state_dict(m.graph, 0)
    for nd in m.graph.nodes:
        if nd.head == 1 and nd.op == "pw":
            for suf in (".weight", ".bias"):
                sd[nd.conv_key + suf] = (sd[nd.conv_key + suf] * np.float32(cool)).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    for k, v in post.items():
        assert hasattr(m, k)
        setattr(m, k, v)
    return m.cuda()


def _eid(c):
    return f"{c[0]}-K{c[1]}" + (f"-size{c[2]}" if c[2] else "") + f"-thresh{c[4]['score_thresh']:g}"


def _raw_labels(m, imgs):
    """the launch labels of one profiled forward_batch, the softmax instantiation's name left in (lp._labels strips it)"""
    L = _lib.lib()
    h = C.c_void_p(m._plan(imgs.device))
    _lib.check(L.dn_profile_begin(h))
    m.forward_batch(imgs, persistent_input=True)
    nseg = len(m.graph.nodes) + 4
    _lib.check(L.dn_profile_end(h, (C.c_float * nseg)(), nseg))
    label, owner = C.create_string_buffer(96), C.c_int32()
    out = []
    for i in range(len(m.graph.nodes)):
        _lib.check(L.dn_profile_op_info(h, i, label, 96, C.byref(owner)))
        out.append(label.value.decode())
    return out


@pytest.mark.parametrize("name,ncls,size,cool,post,ccb_on,seeds", EPILOGUE_CASES, ids=[_eid(c) for c in EPILOGUE_CASES])
def test_softmax_and_decode_in_the_head_launch_across_class_counts(name, ncls, size, cool, post, ccb_on, seeds, monkeypatch):
    """hf_softmax_scores keeps a row in three batches of 32 classes over four lanes, read with an index clamped to K - 1 and guarded by k < K:
    K = 2 (lanes 2 and 3 of a row own no class), 5, the batch edges 32 / 33 and 64 / 65, exact tiles (16, 32, 48, 64, 80), the LDS bound 92, and
    head_fused_kernel<T,softmax> for T = 1 .. 5. Detections with the epilogue equal the logit-writing path + softmax_decode_kernel bit for bit, and
    a graph replay; and, since the two share post_math.h and would share a K-dependent error, they equal the oracle's post-process of the
    device's own head outputs: counts, sorted scores (rtol 1e-5 / atol 1e-7), and labels exactly and boxes (1e-5 / 1e-3) on every image whose
    selection has no near-tie -- at most one of the five may have one."""
    raw = C.CDLL(_lib.LIB_PATH)
    nb = _hist_nb(post["score_thresh"])
    assert (nb + ncls - 1 <= 256) == ccb_on, (nb, ncls)
    res, launches, labels, heads, m = {}, {}, None, None, None
    monkeypatch.setenv("DN_HEAD_SOFTMAX_MINN", "1")          # (by default the epilogue is used from 32 images per chain up)
    for flag in ("0", "1"):
        monkeypatch.setenv("DN_HEAD_SOFTMAX", flag)
        m = _cooled_model(name, ncls, size, cool, post)
        try:
            W, H = m.graph.size
            imgs = torch.stack([torch.from_numpy(synth.images(int(s), 1, H, W)[0]) for s in seeds]).cuda()
            before = raw.dn_debug_head_softmax_launches()
            res[flag] = [t.clone() for t in m.forward_batch(imgs)]
            launches[flag] = raw.dn_debug_head_softmax_launches() - before
            again = m.forward_batch(imgs)                       # graph replay
            for x, y in zip(res[flag], again):
                assert torch.equal(x, y)
            if flag == "1":
                labels = _raw_labels(m, imgs)
                heads = [t.cpu().clone() for t in m.forward_heads(imgs)]
        finally:
            m.release()
    assert launches["0"] == 0 and launches["1"] >= 1, launches
    tcw = _tiles(ncls)[1]
    assert f"head_fused_kernel<{tcw},softmax>" in labels, sorted(set(l for l in labels if l.startswith("head_fused")))
    assert int(res["1"][3].min()) > 0
    for q, what in enumerate(("boxes", "scores", "labels", "counts")):
        assert torch.equal(res["0"][q], res["1"][q]), what
    # the oracle's post-process of the device's own head outputs
    g, p = m.graph, m.graph.post
    assert abs(p["score_thresh"] - post["score_thresh"]) < 1e-12 and p["detections_per_img"] == post["detections_per_img"]
    ref = so.postprocess_detections(heads[0], heads[1], torch.from_numpy(m._lowered.anchors), (g.size[1], g.size[0]), p["score_thresh"], p["nms_thresh"],
                                    p["detections_per_img"], p["topk_candidates"], return_intermediates=True)
    boxes, scores, labs, counts = [t.cpu().numpy() for t in res["1"]]
    risky = []
    for i, d in enumerate(ref):
        cnt = int(counts[i])
        assert cnt == d["labels"].shape[0] <= p["detections_per_img"], (i, cnt, d["labels"].shape[0])
        np.testing.assert_allclose(np.sort(scores[i, :cnt])[::-1], np.sort(d["scores"])[::-1], rtol=1e-5, atol=1e-7)
        mg = so.selection_margins(d["softmax"], d["decoded"], p["score_thresh"], p["nms_thresh"], p["topk_candidates"], p["detections_per_img"])
        if _risky(mg):
            risky.append((i, {k: f"{v:.2e}" for k, v in mg.items()}))
            continue
        assert np.array_equal(labs[i, :cnt], d["labels"]), i
        np.testing.assert_allclose(boxes[i, :cnt], d["boxes"], rtol=1e-5, atol=1e-3)
    print(f"\n{_eid((name, ncls, size, cool, post))}: head_fused_kernel<{tcw},softmax>, nb {nb} (per-class bins {'on' if ccb_on else 'off'}), counts {counts.tolist()}, "
          f"images with a near-tie on the device's logits: {risky}")
    assert len(risky) <= 1, risky


def test_the_epilogue_cases_carry_every_softmax_instantiation():
    assert {_tiles(c[1])[1] for c in EPILOGUE_CASES} == {1, 2, 3, 4, 5}
    assert {c[5] for c in EPILOGUE_CASES} == {True, False}
    assert all(c[1] <= 92 for c in EPILOGUE_CASES)          # the epilogue's LDS bound for 6-anchor levels (test_fused_head_softmax_boundary)


# ---- the 101 / 102 boundary end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls,fused", [(101, True), (102, False)])
def test_fused_head_class_count_boundary(ncls, fused, monkeypatch):
    """K = 101 is the last class count of the fused head launch (20 tiles on 4 waves x 5) and 102 the first on the grouped launches; neither runs
    the softmax epilogue (K > 96). DN_HEAD_FUSE = 0 / 1 give the same detections bit for bit at both."""
    raw = C.CDLL(_lib.LIB_PATH)
    imgs = torch.from_numpy(synth.images(101, 8, 320, 320)).cuda()
    monkeypatch.setenv("DN_HEAD_SOFTMAX_MINN", "1")
    res, nf, ns = {}, {}, {}
    for flag in ("0", "1"):
        monkeypatch.setenv("DN_HEAD_FUSE", flag)
        m = models.load_synthetic(getattr(models, V3)(num_classes=ncls), 0).cuda()
        try:
            f0, s0 = raw.dn_debug_head_fused_launches(), raw.dn_debug_head_softmax_launches()
            res[flag] = [t.clone() for t in m.forward_batch(imgs)]
            nf[flag], ns[flag] = raw.dn_debug_head_fused_launches() - f0, raw.dn_debug_head_softmax_launches() - s0
            for x, y in zip(res[flag], m.forward_batch(imgs)):          # graph replay
                assert torch.equal(x, y)
        finally:
            m.release()
    assert nf["0"] == 0 and (nf["1"] >= 1) == fused and (fused or nf["1"] == 0), nf
    assert ns == {"0": 0, "1": 0}, ns
    assert int(res["1"][3].sum()) > 0 and int(res["1"][2].max()) <= ncls - 1
    for q, what in enumerate(("boxes", "scores", "labels", "counts")):
        assert torch.equal(res["0"][q], res["1"][q]), what
