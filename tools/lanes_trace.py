"""Two-lane forwards vs one lane at B=16: the first tensor (in execution order) that differs."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from omnifusion_amd import _lib as L
from omnifusion_amd.model.spherical_model import spherical_fusion
from omnifusion_amd.model import _engine
from omnifusion_amd.equi_pers.equi2pers_v3 import equi2pers_patches
from omnifusion_amd.weights import make_state_dict
E, F = _engine.Engine, _engine._Forward
oc, ou, og = F.conv, F.up_conv, F.gemm_sh               # (self: the per-forward context; self.e: its engine, whose `trace` collects)
def conv(self, x, key, *a, **k):
    o = oc(self, x, key, *a, **k); self.e.trace.append((key, o)); return o
def up(self, x, key, *a, **k):
    o = ou(self, x, key, *a, **k); self.e.trace.append(("up:" + key, o)); return o
def gemm(self, x, key, *a, **k):
    o = og(self, x, key, *a, **k); self.e.trace.append((key, o)); return o
F.conv, F.up_conv, F.gemm_sh = conv, up, gemm
E.trace = []
net = spherical_fusion(4, 18, (128, 128), (80, 80)).cuda(); net.load_state_dict(make_state_dict(42, 18, False))
B = int(os.environ.get('B', '16'))
rgb = torch.rand((B, 3, 512, 1024), device="cuda")
patches = equi2pers_patches(rgb, 80, 4, 128, layout=L.LAYOUT_BNCHW)
spherical_fusion.LANES = 1
net._eng.trace = []
a1, c1 = net.network(patches, B, True)
ref = {k: v.clone() for k, v in net._eng.trace}; a1 = a1.clone()
torch.cuda.synchronize()
spherical_fusion.LANES = 2
net._eng.trace = []
net.network(patches, B, True)
half = B // 2 * 18
bad = 0
for rep in range(int(os.environ.get('REPS', '600'))):
    for eng, _ in net._lanes: eng.trace = []
    a, c = net.network(patches, B, True)
    torch.cuda.synchronize()
    if torch.equal(a, a1): continue
    bad += 1
    for k, (eng, _) in enumerate(net._lanes):
        for key, v in eng.trace:
            r = ref[key][k * half:(k + 1) * half] if ref[key].shape[0] == B * 18 else ref[key]
            if v.shape != r.shape or not torch.equal(v, r):
                d = (v != r)
                rows = sorted(set(d.nonzero()[:, 0].tolist()))
                print("rep %d lane %d: first differing tensor %-14s shape %s: %d elements, patches %s" % (rep, k, key, tuple(v.shape), int(d.sum()), rows[:5]), flush=True)
                if v.dim() == 4:
                    idx = d.nonzero()
                    print("      rows y %d..%d, x %d..%d, channels %d..%d" % (idx[:, 1].min(), idx[:, 1].max(), idx[:, 2].min(), idx[:, 2].max(), idx[:, 3].min(), idx[:, 3].max()))
                break
print("bad forwards:", bad)
