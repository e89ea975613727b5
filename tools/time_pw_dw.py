"""dev tool: time dn_depthwise_pointwise (pwdirect.hip, the first inverted-residual block) alone on the chip, the body with the global taps
(DN_PW_DW_LDS=0) against the LDS body at several band lengths (DN_PW_DW_BAND).  usage: time_pw_dw.py [images] [band ...]"""
import ctypes as C, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demonet_amd import _lib
L = _lib.lib()
P = lambda t: C.c_void_p(t.data_ptr())
N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
BANDS = [int(v) for v in sys.argv[2:]] or [320, 640, 800, 1280]
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for (h, c, cout, res) in [(160, 16, 16, 1), (150, 32, 16, 0)]:
    xs = [torch.randn(N, h, h, c, device="cuda").half() for _ in range(4)]
    outs = [torch.empty(N, h, h, cout, device="cuda", dtype=torch.half) for _ in range(4)]
    wd = (torch.randn(9, c, device="cuda") / 3).half(); bd = torch.randn(c, device="cuda")
    w = (torch.randn(cout, c, device="cuda") / 4).half(); b = torch.randn(cout, device="cuda")
    call = lambda i: _lib.check(L.dn_depthwise_pointwise(P(xs[i % 4]), P(wd), P(bd), P(w), P(b), P(outs[i % 4]), N, h, h, c, cout, 1, 0, res, stream), "pw_dw")
    for lds, band in [(0, 0)] + [(1, v) for v in BANDS]:
        os.environ["DN_PW_DW_LDS"] = str(lds)
        if band: os.environ["DN_PW_DW_BAND"] = str(band)
        call(0); call(1); torch.cuda.synchronize()
        t = []
        for rep in range(3):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(40): call(i)
            e1.record(); torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 25)
        print(f"n{N} {h}x{h} c{c}->{cout} DN_PW_DW_LDS={lds} band {band:4d}: " + " ".join(f"{v:6.1f}" for v in t) + " us/launch", flush=True)
    os.environ.pop("DN_PW_DW_BAND", None)
