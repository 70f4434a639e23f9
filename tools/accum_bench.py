#!/usr/bin/env python3
"""Gradient accumulation on one GPU: what an optimizer step of ``accum_iter`` micro-batches costs
  (a) eager     Trainer.step per micro-batch as train.py's eager branch drives it (what opt.accum_iter > 1 gave before the captured
                step accepted it): ~1900 launches per micro-step, a host read of the loss and of the gradient norm per micro-step;
  (b) captured  util.misc.GraphedStep with accum_iter micro-steps per window (one forward/backward graph replayed per micro-batch,
                the gated written-first weight gradients, grad norm + AdamW once per window);
  (c) step1     accum_iter x the captured accum_iter = 1 step: the yardstick (AdamW accum_iter times, no gradient read-back).
BASELINE configs[2] (base_as) at B = 64 by default, synthetic tensors resident on the device, device events around every optimizer
step, warm-up as in bench.py, median per optimizer step.

    python tools/accum_bench.py leg --mode eager|captured|step1 [--root TREE] [--config base_as] [--batch 64] [--accum 4]
                                    [--steps 20] [--warmup 3]                     one JSON line
    python tools/accum_bench.py run --parent TREE [--rounds 3] [--out profiles/accum_step.json] [...]
        (a) and (c) from TREE (an export of the parent commit with its own library build: `git archive <commit> | tar -x -C TREE`,
        `make -C TREE/deepavfusion_amd/csrc`), (b) from this tree, alternating a, b, c for --rounds rounds, every leg a fresh
        process under its own time limit; the first leg that fails ends the run.  The run-to-run spread of each figure (max - min
        of its medians) is the margin the comparison is read against.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(root, config, batch, accum):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from deepavfusion_amd.build_model import build_avmae
    from deepavfusion_amd.configs import CONFIGS
    from deepavfusion_amd.util import lr_sched
    from deepavfusion_amd.util.flat import FlatAdamW
    from deepavfusion_amd.util.misc import Trainer
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    cfg = CONFIGS[config]
    torch.manual_seed(0)
    model = build_avmae(cfg).to(dev)
    nd = [n for n, p in model.named_parameters() if 'bias' in n or 'norm' in n]
    groups = lr_sched.param_groups_pretrained(model, 0.05, no_weight_decay_list=nd, image_pt='', audio_pt='')
    opt = FlatAdamW(groups, lr=1.5e-4 * batch * accum / 256, betas=(0.9, 0.95), model=model)
    trainer = Trainer(model, optimizer=opt, accum_iter=accum, use_amp=True, distributed=False)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    image = torch.randn(batch, 3, *cfg.image_size, device=dev, generator=g)
    audio = (torch.randn(batch, 1, *cfg.audio_size, device=dev, generator=g) * 2.0 - 3.0).clamp(-7, 4)
    torch.manual_seed(0)
    return torch, trainer, image, audio


def optimizer_step_fn(a):
    """-> (torch, a callable that runs ONE optimizer step's worth of micro-batches and returns the last losses, trainer)"""
    import math
    if a.mode == 'eager':
        torch, tr, image, audio = build(a.root, a.config, a.batch, a.accum)

        def step():
            for _ in range(a.accum):                      # train.py's eager branch
                with tr.autocast(), tr.autosync():
                    li, la = tr.model(image, audio)[:2]
                    loss = li + la
                if not math.isfinite(loss.item()):
                    raise RuntimeError(f'Loss is {loss.item()}')
                tr.step(loss)
            return li, la
        return torch, step, tr
    accum = a.accum if a.mode == 'captured' else 1
    torch, tr, image, audio = build(a.root, a.config, a.batch, accum)
    from deepavfusion_amd.util.misc import GraphedStep
    gs = GraphedStep(tr, image.shape, audio.shape)

    def step():
        for _ in range(a.accum):
            out = gs(image, audio)
        return out[0], out[1]
    step.gs = gs
    return torch, step, tr


def leg(a):
    torch, step, tr = optimizer_step_fn(a)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    n0 = int(tr.n_steps)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    ev[0].record()
    for i in range(a.steps):
        out = step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps))
    if hasattr(step, 'gs'):
        step.gs.check()
    updates = int(tr.n_steps) - n0
    assert updates == a.steps * (a.accum if a.mode == 'step1' else 1), updates
    loss = float(out[0].detach()) + float(out[1].detach())
    assert loss == loss and abs(loss) != float('inf'), loss
    print(json.dumps({'mode': a.mode, 'config': a.config, 'batch': a.batch, 'accum_iter': a.accum, 'steps': a.steps, 'warmup': a.warmup,
                      'ms_per_optimizer_step_median': round(ms[len(ms) // 2], 3), 'ms_min': round(ms[0], 3), 'ms_max': round(ms[-1], 3),
                      'ms_wall_per_optimizer_step': round(1e3 * wall / a.steps, 3), 'optimizer_updates': updates,
                      'pairs_per_s': round(a.batch * a.accum / (1e-3 * ms[len(ms) // 2]), 1), 'loss': round(loss, 4),
                      'device': torch.cuda.get_device_name(0)}))
    return 0


def run(a):
    me = os.path.abspath(__file__)
    common = ['--config', a.config, '--batch', str(a.batch), '--accum', str(a.accum), '--steps', str(a.steps), '--warmup', str(a.warmup)]
    legs = [('a_eager_parent', 'eager', a.parent), ('b_captured_window', 'captured', ROOT), ('c_step1_x_accum_parent', 'step1', a.parent)]
    res = {k: [] for k, _, _ in legs}
    cmds = {}
    for r in range(a.rounds):
        for key, mode, root in legs:
            cmd = [sys.executable, me, 'leg', '--mode', mode, '--root', root] + common
            cmds[key] = ' '.join(['python', os.path.relpath(me, ROOT), 'leg', '--mode', mode, '--root', os.path.relpath(root, ROOT)] + common)
            p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=a.leg_timeout)      # a fresh process per leg
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                print(f'round {r} {key}: exit code {p.returncode}; nothing more is started', flush=True)
                return 1
            d = json.loads(p.stdout.strip().splitlines()[-1])
            res[key].append(d)
            print(f'round {r} {key:24s} {d["ms_per_optimizer_step_median"]:9.3f} ms per optimizer step (min {d["ms_min"]}, max {d["ms_max"]})', flush=True)
    med = {k: [d['ms_per_optimizer_step_median'] for d in v] for k, v in res.items()}
    mid = {k: sorted(v)[len(v) // 2] for k, v in med.items()}
    spread = {k: round(max(v) - min(v), 3) for k, v in med.items()}
    out = {'what': f'one optimizer step of accum_iter = {a.accum} micro-batches, {a.config} B = {a.batch}, one GPU, device events, median of {a.steps} after {a.warmup} '
                   'warm-up steps per leg, legs alternated a, b, c as fresh processes',
           'device': res['b_captured_window'][0]['device'], 'rounds': a.rounds, 'commands': cmds,
           'ms_per_optimizer_step': med, 'median_of_rounds': mid, 'spread_max_minus_min': spread,
           'b_over_a': round(mid['b_captured_window'] / mid['a_eager_parent'], 4),
           'b_over_c': round(mid['b_captured_window'] / mid['c_step1_x_accum_parent'], 4),
           'b_below_a_by_more_than_the_spread': bool(max(med['b_captured_window']) + max(spread.values()) < min(med['a_eager_parent'])),
           'b_exceeds_c_by_more_than_the_spread': bool(min(med['b_captured_window']) > max(med['c_step1_x_accum_parent']) + max(spread.values())),
           'legs': res}
    print(json.dumps({k: out[k] for k in ('median_of_rounds', 'spread_max_minus_min', 'b_over_a', 'b_over_c',
                                          'b_below_a_by_more_than_the_spread', 'b_exceeds_c_by_more_than_the_spread')}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        prev = json.load(open(a.out)) if os.path.exists(a.out) else {}
        prev['accum_bench'] = out
        json.dump(prev, open(a.out, 'w'), indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['leg', 'run'])
    ap.add_argument('--mode', choices=['eager', 'captured', 'step1'], default='captured')
    ap.add_argument('--root', default=ROOT, help='the tree whose package the leg imports')
    ap.add_argument('--parent', default=None, help='run: an export of the parent commit, built')
    ap.add_argument('--config', default='base_as')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--accum', type=int, default=4)
    ap.add_argument('--steps', type=int, default=20, help='timed optimizer steps per leg')
    ap.add_argument('--warmup', type=int, default=3, help='optimizer steps before the clock')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--leg-timeout', type=int, default=240)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.what == 'run':
        if not a.parent or not os.path.isdir(a.parent):
            ap.error('run needs --parent TREE')
        a.parent = os.path.abspath(a.parent)
        return run(a)
    return leg(a)


if __name__ == '__main__':
    sys.exit(main())
