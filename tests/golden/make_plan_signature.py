"""Generator of tests/golden/plan_signature.json: what the native plan decides for each factory model, pinned so that a change
of plan.hip's host code that should not move anything can be checked against it (tests/test_gpu_plan_signature.py).

Per configuration (a factory model plus the knobs set while its plan is built and run):
  ops      the (kernel label, owner op) that dn_profile_op_info reports for every op after one profiled forward, at n = 16
           and n = 64: which ops share a launch, which kernel each launch took, whose event segment holds it
  ws       dn_workspace_bytes at n = 1, 16, 32, 64, 128
  tensors  [tensor id, byte offset, bytes] of every materialised workspace tensor at n = 16 (dn_tensor_ptr)
Needs the GPU (plans upload their weights). Run on the GPU box: python tests/golden/make_plan_signature.py"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "plan_signature.json")
MODELS = ["ssdlite320_mobilenet_v3_large", "ssd_lite_mobilenet_v2", "ssd300_vgg16", "ssd512_vgg16"]
KNOBS = [{"DN_SE_IN_DW": "1"}, {"DN_PW_DW": "2"}, {"DN_HEAD_FUSE": "0"}, {"DN_TAIL": "0"}, {"DN_EXPDW": "0"}, {"DN_WS_REUSE": "0"}]
CONFIGS = [(m, {}) for m in MODELS] + [("ssdlite320_mobilenet_v3_large", k) for k in KNOBS]
PROFILE_N = (16, 64)
WS_N = (1, 16, 32, 64, 128)


def config_key(name, env):
    return " ".join([name] + [f"{k}={v}" for k, v in sorted(env.items())])


def _signature(name):
    import torch
    from demonet_amd import _lib, models, synth
    L = _lib.lib()
    dev = torch.device("cuda:0")
    m = models.load_synthetic(getattr(models, name)(num_classes=91), 0).to(dev)
    W, H = m.graph.size
    h = C.c_void_p(m._plan(dev))
    label, owner = C.create_string_buffer(96), C.c_int32()
    ops = {}
    for n in PROFILE_N:
        imgs = torch.from_numpy(synth.images(7, n, H, W)).to(dev)
        _lib.check(L.dn_profile_begin(h))
        m.forward_batch(imgs, persistent_input=True)
        nseg = len(m.graph.nodes) + 4
        _lib.check(L.dn_profile_end(h, (C.c_float * nseg)(), nseg))
        row = []
        for i in range(len(m.graph.nodes)):
            _lib.check(L.dn_profile_op_info(h, i, label, 96, C.byref(owner)))
            row.append([label.value.decode(), owner.value])
        ops[str(n)] = row
    torch.cuda.synchronize()
    ws = {str(n): int(L.dn_workspace_bytes(h, n)) for n in WS_N}
    base = m._buffers_for(16, H, W, dev)["ws"].data_ptr()
    ptr, size = C.c_void_p(), C.c_size_t()
    tensors = []
    for tid in range(len(m.graph.tensors)):
        if L.dn_tensor_ptr(h, C.c_void_p(base), 16, tid, C.byref(ptr), C.byref(size)) == 0:
            tensors.append([tid, ptr.value - base, size.value])
    m.release()
    return {"ops": ops, "ws": ws, "tensors": tensors}


def signature(name, env):
    """The signature of one configuration; `env` is set around plan creation and the forwards (some knobs are read per launch)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _signature(name)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


if __name__ == "__main__":
    sig = {config_key(name, env): signature(name, env) for name, env in CONFIGS}
    with open(OUT, "w") as f:
        json.dump(sig, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
