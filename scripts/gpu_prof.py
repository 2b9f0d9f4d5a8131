"""Per-phase shader-clock breakdown of the mixnet kernel (debug aid; not the bench)."""
import sys, time, os
import numpy as np, torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [R, os.path.join(R, 'tests')]
from conftest import synth_mixnet_inputs
from cmix_amd import engine as E

T = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
probs, sel, bits = synth_mixnet_inputs(T, seed=1)
net = E.MixNet(0)
dp = torch.from_numpy(probs).cuda()
ds = torch.from_numpy((sel & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).cuda()
db = torch.from_numpy(bits).cuda()
net.run(dp, ds, db); torch.cuda.synchronize()
print('plain: kernel %.2f ms  %.2f us/bit' % (net.last_kernel_ms(), net.last_kernel_ms() * 1e3 / T))
net.profile(True)
net.run(dp, ds, db); torch.cuda.synchronize()
ms = net.last_kernel_ms()
pr = net.profile(False)
# the gather wave's phases
names = ['wait scout', 'row state + decay', 'wait the 26 sums (helpers)', 'extras chain', 'u + publish (global)',
         'tail handoff + extras upd', '-', '-', '-', '-', '-', '-', 'wait tail_done(t-1)', '-', '-', '-']
print('speculation:', net.spec_stats())
print('re-runs:', net.spec_rerun_stats())   # how the re-runs were executed: resolved at the mid-point / second half serial
if int(os.environ.get('CMX_MIXNET_DBG', '0')) & 4:   # the tail's two waves
    names[6:12] = ['TAIL A: row switch + prefetch', 'TAIL A: wait slot + tail_in', 'TAIL A: layer 1 (dot + chain) + hand-over', '-', 'TAIL A: layer-1 updates', 'TAIL A: loop top + wait scout']
    names[13:16] = ['TAIL B: SSE touches + wait hand-over', 'TAIL B: layer 2 + SSE + output', 'TAIL B: layer-2 update + publish']
tot = sum(pr[:6]) + pr[12]
print('profiled: kernel %.2f ms  %.2f us/bit; total ticks/bit %.0f' % (ms, ms * 1e3 / T, tot / T))
for n, v in zip(names, pr):
    if n == 'simd ids':
        continue
    print('  %-34s %9.0f ticks/bit  %5.1f%%' % (n, v / T, 100.0 * v / tot))
