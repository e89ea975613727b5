"""dev tool: phase timing of dw_kernel (s_memrealtime stamps, 100 MHz; needs the stamped build: python -m demonet_amd.build --stamps, then
DEMONET_HIP_LIB=demonet_amd/lib/libdemonet_hip_stamps.so) on the depthwise launches that carry the SE tail, under DN_DW_WLDS = 0 and 1.
Per workgroup: copy (weights to LDS + barrier; nothing for the per-thread body) | rows | store | reduce + publish | ticket | tail (the image's last workgroup)."""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demonet_amd import _lib
L = _lib.lib()
L.dn_debug_dw_stamps.argtypes = [C.c_void_p]
P = lambda t: C.c_void_p(t.data_ptr())
N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for (h, c, k, s, sq) in [(80, 72, 5, 2, 24), (40, 120, 5, 1, 32)]:
    pad = (k - 1) // 2
    ho = (h + 2 * pad - k) // s + 1
    x = torch.randn(N, h, h, c, device="cuda").half(); out = torch.empty(N, ho, ho, c, device="cuda", dtype=torch.half)
    w = (torch.randn(k * k, c, device="cuda") / k).half(); b = torch.randn(c, device="cuda")
    blocks = L.dn_depthwise_pool_blocks(h, h, c, k, s, pad)
    rows = torch.zeros(N, blocks, c, device="cuda"); scale = torch.zeros(N, c, device="cuda"); cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    w1t = torch.randn(c, sq, device="cuda").half(); w2t = torch.randn(sq, c, device="cuda").half()
    b1 = torch.randn(sq, device="cuda"); b2 = torch.randn(c, device="cuda")
    call = lambda: _lib.check(L.dn_depthwise_conv_pool(P(x), P(w), P(b), P(out), N, h, h, c, k, s, pad, 3, P(rows), P(w1t), P(b1), P(w2t), P(b2), P(scale), P(cnt), sq, stream), "dw")
    for knob in ("0", "1"):
        os.environ["DN_DW_WLDS"] = knob
        call(); call(); torch.cuda.synchronize()
        st = torch.zeros(N * blocks * 8, dtype=torch.int64, device="cuda")
        L.dn_debug_dw_stamps(P(st))
        call(); torch.cuda.synchronize()
        L.dn_debug_dw_stamps(None)
        t = st.cpu().numpy().reshape(N * blocks, 8).astype(np.float64) * 0.01      # us
        d = np.diff(t[:, :6], axis=1)
        last = t[:, 6] > 0
        print(f"{h}x{h} c{c} k{k}s{s} n{N} DN_DW_WLDS={knob}: {N * blocks} workgroups; per workgroup us: copy {d[:, 0].mean():.2f} rows {d[:, 1].mean():.2f} store {d[:, 2].mean():.2f} "
              f"reduce+publish {d[:, 3].mean():.2f} ticket {d[:, 4].mean():.2f} life {(t[:, 5] - t[:, 0]).mean():.2f}; tail {(t[last, 6] - t[last, 5]).mean():.2f} x {int(last.sum())}; "
              f"span {t[:, :7].max() - t[:, 0].min():.2f}, last ticket at {t[:, 5].max() - t[:, 0].min():.2f}, last tail start - end {t[last, 5].max() - t[:, 0].min():.2f} - {t[last, 6].max() - t[:, 0].min():.2f}", flush=True)
