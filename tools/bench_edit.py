"""Wall-clock split of the editing modes between the compose front end (dfx_compose_latents: code lerp / swap, aligner, anchor edit,
seg ids, per-point gathers) and the persistent chain, at the shipped size:

    python tools/bench_edit.py [B] [K] [T] [--reps R] [--precision bf16|f32]     (defaults 128 10 100, 3 reps)

B shapes x K edits per shape = B*K rows of 2048 points, synthetic weights.  Prints one line per mode (interpolate, mix, drift) with the
median milliseconds of each part and the end-to-end rate in edited shapes/s.  Numbers only; not part of bench.py.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import numpy as np
import torch

from difffacto_amd import editing, synth
from difffacto_amd.modules import decode
from generate import build

_pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in ("--reps", "--precision")]
B = int(_pos[0]) if len(_pos) > 0 else 128
K = int(_pos[1]) if len(_pos) > 1 else 10
T = int(_pos[2]) if len(_pos) > 2 else 100
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
PREC = sys.argv[sys.argv.index("--precision") + 1] if "--precision" in sys.argv else "bf16"
N = 2048

enc, diff = build("gen_chair", T, PREC, 0)
W = synth.make_latent_weights(0)
W.update({"encoder." + k: v for k, v in synth.make_pointnet_v2_weights(0).items()})
enc.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
diff.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_denoiser_weights(0).items()})
enc, diff = enc.cuda().eval(), diff.cuda().eval()
J = enc.n_class
g = torch.Generator().manual_seed(0)
codes = enc.sampler().flow_reverse(torch.randn(B, enc.zdim, J, generator=g).cuda())
valid = torch.ones(B, J, device="cuda")
noise_b = torch.randn(B, enc.part_aligner.noise_dim, generator=g).cuda()
noise_bk = torch.randn(B * K, enc.part_aligner.noise_dim, generator=g).cuda()
rows = editing.repeat_rows(B, K)
vk = valid.repeat_interleave(K, 0)

code_a, code_b = editing.interpolation_recipe(B, K, J, 2, np.roll(np.arange(B), -1))
alpha = editing.interpolation_alpha(B, K, J, 2, torch.linspace(0, 1, steps=K)).cuda()
donors = np.stack([np.roll(np.arange(B), -j) for j in range(J)], 1)
s, l = editing.drift_factors(B, K, J, torch.linspace(1, 5, steps=K))
MODES = {
    "interpolate": lambda: enc.compose_latents(codes, code_a, vk, N, code_b=code_b, alpha=alpha, noise_src=noise_b, noise_row=rows),
    "mix": lambda: enc.compose_latents(codes, editing.mixing_recipe([donors[:, j] for j in range(J)], K), vk, N, noise_src=noise_bk),
    "drift": lambda: enc.compose_latents(codes, np.repeat(rows[:, None], J, 1), vk, N, noise_src=noise_b, noise_row=rows,
                                         mean_scale=s.cuda(), logvar_shift=l.cuda()),
}


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


print(f"editing front end vs chain: B={B} shapes x K={K} = {B * K} rows, N={N}, T={T} DDPM steps, {PREC}, median of {REPS}")
for name, compose in MODES.items():
    ctx, mpp, lpp, seg, v, _ = compose()                       # warm-up (handles, workspaces)
    decode(diff, ctx, seg, valid_id=v, seed=0)
    fe, ch = [], []
    for r in range(REPS):
        (ctx, mpp, lpp, seg, v, _), t_fe = timed(compose)
        _, t_ch = timed(lambda: decode(diff, ctx, seg, valid_id=v, seed=r))
        fe.append(t_fe), ch.append(t_ch)
    t_fe, t_ch = float(np.median(fe)), float(np.median(ch))
    print(f"{name:12s} front end {t_fe:8.2f} ms  chain {t_ch:9.2f} ms  front-end share {100 * t_fe / (t_fe + t_ch):5.2f} %  "
          f"{B * K / ((t_fe + t_ch) / 1e3):8.1f} shapes/s (front end alone {B * K / (t_fe / 1e3):9.1f} shapes/s)")
