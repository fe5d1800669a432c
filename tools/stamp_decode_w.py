"""diagnostic: per-phase WORK cycles (barrier waits excluded) of the two wave groups of the wave-specialised BL6 decode kernel
   (each group's first wave, and group A's wave 1, which stages the sampling noise)
   (needs the -DSWN_STAMP build: make -C shallow_wavenet_amd/csrc stamp ;
    SWN_HIP_LIB=shallow_wavenet_amd/libswn_hip_stamp.so python tools/stamp_decode_w.py)"""
import sys, os
import torch
_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, _R)
from shallow_wavenet_amd import config as C
from shallow_wavenet_amd.runtime import HipNet
from shallow_wavenet_amd.synth import synth_state_dict, synth_aux

# eight barriers per step: phase 0 is the previous step's tail (out_2, head, sample, h0 in every wave of group A) + layer 0
names = ["tail+L0", "L1", "L2", "L3", "L4", "L5", "skip-fin", "out_1"]
cfg = C.bl6_laplace(1, 0)
sd = synth_state_dict(cfg, seed=1, flavor="trained", identity_scale_in=True)
net = HipNet.from_state_dict(cfg, sd, "cuda:0")
Tf = 40
n_steps = Tf * cfg.U
aux = torch.from_numpy(synth_aux(cfg, 1, Tf)).cuda()
noise = torch.empty(1, n_steps, 1).uniform_(-0.4999, 0.5).cuda()
for _ in range(2):
    out, heads = net.decode(aux, n_steps, noise, want_heads=True, variant=2)
torch.cuda.synchronize()
h = heads.flatten()[:50].cpu().numpy()
print("step total (group A clock): %.0f ticks" % h[9])
for k, n in enumerate(names):
    print("   %-10s A works %7.0f   B works %7.0f   A's wave 1 %7.0f" % (n, h[k], h[10 + k], h[30 + k]))
print("   (of tail+L0: the tail, group A %7.0f, its wave 1 %7.0f)" % (h[8], h[38]))
print("   sum        A %7.0f   B %7.0f   A's wave 1 %7.0f" % (h[:8].sum(), h[10:18].sum(), h[30:38].sum()))
# group B, from the barrier's release until the first out_skip weight register of the slice in flight has landed
print("   B's wait for its slice:  " + "  ".join("%s %.0f" % (n, h[20 + k]) for k, n in enumerate(names[1:7])))
# group B, its wait for the out_skip loads it requested at the head of the phase (the last of the previous phase's slice), taken
# in front of their first use three quarters of a phase later; includes two s_memtime round trips
print("   B's wait for the head-of-phase loads:  " + "  ".join("%s %.0f" % (n, h[44 + k]) for k, n in enumerate(names[1:6])))
