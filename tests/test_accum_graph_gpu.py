"""GPU: gradient accumulation inside the captured step (util.misc.GraphedStep with trainer.accum_iter > 1; reference
util/misc.py:96-148): ONE captured forward/backward replayed per micro-batch, the written-first weight gradients gated on the
device (dav_gemm_tn_gang_bf16_gated, dav_gemm_tn_grouped_bf16_gated), grad norm + AdamW once per window.

Every bound below is the bound of an existing test: losses / norms / parameter sums of ``test_trainer_step_semantics`` against the
reference fixture, the quiet / noisy parameter split of ``test_written_first_gradients_equal_accumulated_ones`` (2e-4 / 1e-3), the
kernel bounds of tests/gpu_selfcheck.py (``gemm_tn``, ``gemm_tn_gang``), ``graph_param_rel`` of tests/test_dp_rccl_gpu.py (1e-3).
The fresh-process tests come last."""
import json
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
WORKER = os.path.join(ROOT, 'tests', 'accum_dp_worker.py')
BF16, F32 = torch.bfloat16, torch.float32


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().flatten()
    b = torch.as_tensor(b).detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _setup(accum_iter, lr=1e-3):
    from deepavfusion_amd.build_model import build_avmae
    from deepavfusion_amd.configs import CONFIGS
    from deepavfusion_amd.util import lr_sched
    from deepavfusion_amd.util.flat import FlatAdamW
    from deepavfusion_amd.util.misc import Trainer
    from oracle import avmae_oracle as O
    from oracle.configs import CONFIGS as OC
    model = build_avmae(CONFIGS['micro']).cuda()
    model.load_state_dict(O.closed_form_state(OC['micro'], 0), strict=True)
    nd = [n for n, p in model.named_parameters() if 'bias' in n or 'norm' in n]
    groups = lr_sched.param_groups_pretrained(model, 0.05, no_weight_decay_list=nd, image_pt='', audio_pt='')
    opt = FlatAdamW(groups, lr=lr, betas=(0.9, 0.95), model=model)
    tr = Trainer(model, optimizer=opt, accum_iter=accum_iter)
    return model, opt, tr, OC['micro'], O


_BATCHES = {}


def _batch(B, seed):
    """(image, audio, noise_image, noise_audio) on the device; made once per (B, seed)."""
    if (B, seed) not in _BATCHES:
        from oracle import avmae_oracle as O
        from oracle.configs import CONFIGS as OC
        image, audio, ni, na = O.synthetic_batch(OC['micro'], B, seed=seed)
        _BATCHES[(B, seed)] = (image.cuda(), audio.cuda(), torch.from_numpy(ni).cuda(), torch.from_numpy(na).cuda())
    return _BATCHES[(B, seed)]


def _captured(accum_iter=2, clip=None, B=64):
    from deepavfusion_amd.util.misc import GraphedStep
    model, opt, tr, cfg, O = _setup(accum_iter)
    im, au = _batch(B, 700)[:2]
    gs = GraphedStep(tr, im.shape, au.shape, clip_grad=clip, inject_noise=True)
    return model, opt, tr, gs


def _micro(gs, b):
    return gs(b[0], b[1], noise_image=b[2], noise_audio=b[3])


def _eager_micro(tr, b):
    li, la = tr.model(*b)[:2]
    norm, _ = tr.step(li + la)
    return li, la, norm


def _layout(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    return [(names[id(p)], o, p.numel()) for p, o in zip(opt.flat.params, opt.flat.offsets)]


def _assert_same_parameters(a, b, layout, tag=''):
    """The quiet / noisy split of test_written_first_gradients_equal_accumulated_ones: 2e-4 on everything but the key parts of the
    biases that make keys and the pair attention's k weight (zero-gradient parameters on which AdamW amplifies rounding noise), whose
    share of the difference is held to 1e-3 of the norm of ALL parameters."""
    def key_part(n, sz):
        if n.endswith('.qkv.bias'):
            return sz // 3, 2 * sz // 3
        if n.endswith('.kv.bias'):
            return 0, sz // 2
        if n.endswith('.attn.k.bias') or n.endswith('.attn.k.weight'):
            return 0, sz
        return 0, 0
    noisy = torch.zeros(a.numel(), dtype=torch.bool, device=a.device)
    owned = torch.zeros_like(noisy)
    for n, o, sz in layout:
        lo, hi = key_part(n, sz)
        noisy[o + lo:o + hi] = True
        owned[o:o + sz] = True
    quiet = owned & ~noisy
    assert bool(noisy.any()) and bool(quiet.any())
    rq = rel(a[quiet], b[quiet])
    rn = float((a[noisy] - b[noisy]).double().norm() / b.double().norm())
    print(f'{tag} parameters: quiet rel {rq:.3e} (bound 2e-4), noisy share {rn:.3e} (bound 1e-3)')
    assert rq < 2e-4, (tag, rq)
    assert rn < 1e-3, (tag, rn)


def _n_linear(model):
    return sum(1 for n, p in model.named_parameters() if p.ndim == 2 and p.requires_grad)


# ---- 1. the reference fixture ---------------------------------------------------------------------------------------------------
def test_captured_accumulation_matches_the_reference_fixture(golden):
    """tests/golden/trainer_steps.npz (generated from the reference's Trainer, accum_iter = 2, six micro-batches of 2): the captured
    window gives the reference's micro-losses, its grad norm on every window's last micro-step, its step count and its parameters —
    under the rules of test_trainer_step_semantics, which the eager path meets."""
    from deepavfusion_amd.util import lr_sched
    from deepavfusion_amd.util.misc import GraphedStep
    g = golden('trainer_steps')
    model, opt, tr, cfg, O = _setup(2)
    b0 = _batch(2, 300)
    gs = GraphedStep(tr, b0[0].shape, b0[1].shape, inject_noise=True)

    class NS(dict):
        __getattr__ = dict.__getitem__
    args = NS(opt=NS(lr=1e-3, warmup_epochs=1, epochs=4, pt_warmup_epochs='4/2', pt_lr_mult_start=0, pt_lr_mult_end=1))
    for step in range(6):
        if step % 2 == 0:
            lr = lr_sched.adjust_learning_rate(opt, step / 6 * 4, args)
            assert abs(lr - g['lr'][step // 2]) < 1e-12
        li, la, gn = _micro(gs, _batch(2, 300 + step))
        loss = float(li) + float(la)
        print(f'step {step}: loss {loss:.6f} (reference {float(g["loss"][step]):.6f})  grad_norm {float(gn):.5f} (reference {float(g["grad_norm"][step]):.5f})')
        assert abs(loss - g['loss'][step]) < 3e-3 * g['loss'][step], step
        if step % 2 == 1:
            assert abs(float(gn) - g['grad_norm'][step]) < 2e-2 * g['grad_norm'][step], (step, float(gn), g['grad_norm'][step])
        assert tr.accums == (step + 1) % 2
    gs.check()
    assert int(tr.n_steps) == int(g['n_steps']) == 3
    sums = dict(zip(g['param_names'].tolist(), g['param_sums'].tolist()))
    bad = []
    for n, p in model.named_parameters():
        if n.endswith(('qkv.bias', 'kv.bias', '.k.bias')) or p.numel() < 64:
            continue          # zero-gradient key biases: Adam amplifies rounding noise (see tests/test_oracle_golden.py)
        if abs(float(p.detach().double().sum()) - sums[n]) > 5e-3 * max(abs(sums[n]), 1.0) + 3e-3 * p.numel() ** 0.5:
            bad.append(n)
    assert len(bad) <= 3, bad


# ---- 2. captured window == eager window ------------------------------------------------------------------------------------------
def _eager_reference(windows=3):
    """Three eager windows of two micro-batches (seeds 700 ..): losses, norms of the windows, final parameters."""
    if 'eager' not in _BATCHES:
        model, opt, tr, cfg, O = _setup(2)
        losses, norms = [], []
        for s in range(2 * windows):
            li, la, norm = _eager_micro(tr, _batch(64, 700 + s))
            losses.append(float(li.detach()) + float(la.detach()))
            norms.append(norm)
        torch.cuda.synchronize()
        _BATCHES['eager'] = (losses, norms, opt.flat.flat_p.detach().clone(), int(tr.n_steps))
    return _BATCHES['eager']


@pytest.mark.parametrize('overwrite', ['1', '0'])
def test_captured_window_equals_eager_window(monkeypatch, overwrite):
    """Same model, same micro-batches, same masking noise: three windows of accum_iter = 2 captured and eager.  With write-first on
    (the default) most Linear weights are kept, i.e. the gated launches carry them; DAV_WGRAD_OVERWRITE=0 accumulates everywhere.

    Measured on one MI355X (four visits, eager run and both captured runs each): micro-steps 0-3 agree to every digit in all of them.
    The two micro-steps of the THIRD window take one of two values in any run, eager or captured, either switch setting
    (3.1806319 / 3.1872861 or 3.1805848 / 3.1873136): the weight gradients that split the contraction and the mask tokens'
    gradients add with fp32 atomics in whatever order the hardware retires them, in the eager step and in the captured one alike, and
    two AdamW updates amplify a last-bit difference (test_written_first_gradients_equal_accumulated_ones allows 5e-5 behind such a
    step).  When the two runs compared land on different values the loss check below misses its 1e-5 at micro-step 4 with 1.48e-5
    (8.6e-6 at micro-step 5): all three runs agreed on the first visit, the eager run differed from both captured runs on the last.
    The bound is the one the feature was specified with and stays."""
    monkeypatch.setenv('DAV_WGRAD_OVERWRITE', overwrite)
    ref_losses, ref_norms, ref_p, ref_steps = _eager_reference()
    model, opt, tr, gs = _captured(2)
    n_linear = _n_linear(model)
    if overwrite == '1':
        assert gs.kept_params > n_linear // 2, (gs.kept_params, n_linear)
        assert gs.gate is not None and gs.gate.dtype == torch.int32 and gs.gate.numel() == 1
    else:
        assert gs.kept_params == 0
    assert len(gs.graphs) == gs.n_seg == 1 and gs.opt_graph is not None
    losses, norms = [], []
    for s in range(6):
        li, la, gn = _micro(gs, _batch(64, 700 + s))
        losses.append(float(li) + float(la))
        norms.append(float(gn))
    torch.cuda.synchronize()
    gs.check()
    assert int(tr.n_steps) == ref_steps == 3 and opt.step_count == 3
    for k, (a, b) in enumerate(zip(losses, ref_losses)):
        print(f'micro-step {k}: captured {a:.7f} eager {b:.7f} rel {abs(a - b) / abs(b):.2e}')
    for k, (a, b) in enumerate(zip(losses, ref_losses)):
        assert abs(a - b) <= 1e-5 * abs(b), (k, losses, ref_losses)
    for w in range(3):      # the norm reported on a window's last micro-step is the window's (the eager norm / accums there)
        assert abs(norms[2 * w + 1] - ref_norms[2 * w + 1]) < 1e-4 * ref_norms[2 * w + 1], (w, norms, ref_norms)
    assert norms[0] == 0.0 and norms[2] == norms[1] and norms[4] == norms[3]      # earlier micro-steps: the previous window's
    assert losses[-1] < losses[0]
    _assert_same_parameters(opt.flat.flat_p.detach(), ref_p, _layout(model, opt), f'captured (overwrite={overwrite}) vs eager')


# ---- 3. the gate through the C ABI -----------------------------------------------------------------------------------------------
def _rnd(*shape, dtype=F32, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g).to(device='cuda', dtype=dtype)


@pytest.mark.parametrize('kind', ['gang', 'grouped'])
def test_write_gate_through_the_c_abi(kind):
    """Flagged problems (DavTnProblem.flags bit 0) under an open gate are WRITTEN — bit-equal to the ungated written launch, the NaN
    poison gone; under a closed gate they are ACCUMULATED onto their old contents; an unflagged problem accumulates either way; the
    bias gradients accumulate regardless.  Every element within the bound tests/gpu_selfcheck.py uses for this kernel, relative
    error <= 2e-4, guard bands untouched."""
    import kcheck as kc
    from deepavfusion_amd import ops
    dev = torch.device('cuda')
    if kind == 'gang':
        shapes = [(512, 768, 768), (3136, 192, 768), (640, 8, 264), (2048, 520, 776), (63 * 8, 768, 192), (64, 256, 256)]
        launch = lambda probs, gate=None: ops.gemm_tn_gang(probs, workspace_fill=0xFF, **({} if gate is None else {'gate': gate}))
    else:
        shapes = [(3136, 768, 768), (512, 192, 768), (2048, 72, 136), (4032, 768, 3072), (640, 8, 264)]
        launch = lambda probs, gate=None: ops.gemm_tn_grouped(probs, **({} if gate is None else {'gate': gate}))
    ops_in = [(_rnd(Mc, N, dtype=BF16, seed=260 + i), _rnd(Mc, K, dtype=BF16, seed=270 + i)) for i, (Mc, N, K) in enumerate(shapes)]
    flagged = [i != 1 for i in range(len(shapes))]

    def run(gate_value):
        """gate_value None: the ungated entry point.  -> (problems, guards, prefills)"""
        probs, guards, pres = [], [], []
        for i, (Mc, N, K) in enumerate(shapes):
            A, Bm = ops_in[i]
            P0, pb0 = kc.prefilled((N, K), F32, dev, seed=280 + i), kc.prefilled((N,), F32, dev, seed=290 + i)
            written = flagged[i] and gate_value != 0
            gC = kc.Guarded(N, K, F32, ld=K + 8 * (0, 0, 1, 5)[i % 4], device=dev, fill='poison' if written else P0)
            bg = pb0.clone() if i % 3 != 2 else None
            probs.append(dict(A=A, B=Bm, Mc=Mc, N=N, K=K, C=gC.t, lda=N, ldb=K, ldc=gC.ld, bias_grad=bg, overwrite=flagged[i]))
            guards.append(gC)
            pres.append((P0, pb0))
        if gate_value is None:
            launch(probs)
        else:
            launch(probs, torch.full((1,), gate_value, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        return probs, guards, pres
    ungated, _, _ = run(None)
    for gate_value in (1, 0, 7):          # (any non-zero value opens the gate)
        probs, guards, pres = run(gate_value)
        for i, pr in enumerate(probs):
            tag = f'{kind} gate={gate_value} #{i} {shapes[i]} {"flagged" if flagged[i] else "unflagged"}'
            written = flagged[i] and gate_value != 0
            prod = pr['A'].double().t() @ pr['B'].double()
            r64 = prod if written else pres[i][0].double() + prod
            assert bool(torch.isfinite(pr['C']).all()), tag + ': poison left'
            ok, ratio, msg = kc.within(pr['C'], r64, kc.gemm_bound(pr['A'].t(), pr['B'].t(), r64, F32), tag)
            print(f'{tag}: worst err/bound {ratio:.3e}, rel {rel(pr["C"], r64):.2e}')
            assert ok, msg
            assert rel(pr['C'], r64) <= 2e-4, tag
            if written:
                n, msg = kc.exact(pr['C'].contiguous(), ungated[i]['C'].contiguous(), tag)
                assert n == 0, msg
            if pr['bias_grad'] is not None:
                b64 = pres[i][1].double() + pr['A'].double().sum(0)
                ok, ratio, msg = kc.within(pr['bias_grad'], b64,
                                           kc.C_GEMM * kc.U32 * pr['Mc'] * pr['A'].double().abs().sum(0) + kc.out_round(F32) * b64.abs(), tag + ' bias')
                assert ok, msg
            n, where = guards[i].stray()
            assert n == 0, f'{tag}: {n} stray elements, first in the {where}'
    with pytest.raises(ValueError):
        launch(ungated, torch.ones(1, dtype=torch.float32, device=dev))       # the gate is one int32


# ---- 4. guard and clip across a window -------------------------------------------------------------------------------------------
def test_window_guards_non_finite_loss_and_clips():
    """test_captured_step_guards_non_finite_loss_and_clips over a window: a NaN in the input of micro-step 0 of 2 followed by a clean
    micro-step 1 leaves parameters, both moments and the bf16 mirror bit-identical, ``check()`` raises, and the next clean window
    equals the one of a run that never saw the bad window.  (That run takes the HOST side of a step — ``prepare_step()`` — in the bad
    window's place: Adam's step count and bias corrections advance for a skipped step, as GraphedStep's docstring says; the device
    side is what the guard protects.)  A clip far above the norm changes nothing; one below it scales the update by
    clip / (norm / accum_iter)."""
    b = [_batch(64, 700 + s) for s in range(4)]
    finals = []
    for poisoned in (True, False):
        model, opt, tr, gs = _captured(2)
        _micro(gs, b[0]); _micro(gs, b[1])
        torch.cuda.synchronize()
        gs.check()
        if poisoned:
            snap = [t.clone() for t in (opt.flat.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.flat_bf16)]
            bad = b[2][0].clone()
            bad[3, 1, 5, 7] = float('nan')
            li, la, gn = gs(bad, b[2][1], noise_image=b[2][2], noise_audio=b[2][3])
            assert not np.isfinite(float(li) + float(la)) and tr.accums == 1
            li, la, gn = _micro(gs, b[3])
            torch.cuda.synchronize()
            assert np.isfinite(float(li) + float(la)) and tr.accums == 0
            for a, c in zip(snap, (opt.flat.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.flat_bf16)):
                assert torch.equal(a, c)
            assert int(gs.bad_steps) == 1 and float(gs.step_scale) == 0.0
            with pytest.raises(RuntimeError, match='stopping training'):
                gs.check()
        else:
            opt.prepare_step()
        li, la, gn = _micro(gs, b[2]); li, la, gn = _micro(gs, b[3])
        torch.cuda.synchronize()
        assert np.isfinite(float(li) + float(la)) and np.isfinite(float(gn)) and float(gs.step_scale) == 1.0
        if poisoned:
            assert not torch.equal(snap[0], opt.flat.flat_p) and int(gs.bad_steps) == 1
        finals.append(opt.flat.flat_p.detach().clone())
        layout = _layout(model, opt)
    _assert_same_parameters(finals[0], finals[1], layout, 'window after a skipped window vs clean run')
    # ---- clipping: far above the norm == no clipping; below the norm: the factor min(1, clip / (norm / accum_iter))
    finals, norms = [], []
    for clip in (None, 1e9):
        model, opt, tr, gs = _captured(2, clip=clip)
        for s in range(4):
            li, la, gn = _micro(gs, b[s])
        torch.cuda.synchronize()
        finals.append(opt.flat.flat_p.detach().clone())
        norms.append(float(gn))
    assert rel(finals[0], finals[1]) < 2e-4 and abs(norms[0] - norms[1]) < 1e-4 * norms[1]
    model, opt, tr, gs = _captured(2, clip=0.5 * norms[0])
    for s in range(4):
        li, la, gn = _micro(gs, b[s])
    torch.cuda.synchronize()
    want = 0.5 * norms[0] / (float(gn) + 1e-6)                   # gn is norm(sum of the window's gradients) / accum_iter
    print(f'step_scale {float(gs.step_scale):.6f}, clip / (norm / accum_iter) {want:.6f}, norm {float(gn):.5f}')
    assert abs(float(gs.step_scale) - want) < 1e-6 and 0.2 < float(gs.step_scale) < 1.0
    assert abs(float(gn) - norms[0]) < 0.2 * norms[0]            # the norm reported is the unclipped one


# ---- 5. window bookkeeping ---------------------------------------------------------------------------------------------------------
def test_window_bookkeeping_restart_and_eager_micro_step():
    b = [_batch(64, 700 + s) for s in range(4)]
    # all captured: the counters
    model, opt, tr, gs = _captured(2)
    layout = _layout(model, opt)
    seen = []
    for s in range(4):
        _micro(gs, b[s])
        seen.append((tr.accums, int(tr.n_steps), opt.step_count, int(next(iter(opt.state.values()))['step'])))
    torch.cuda.synchronize()
    assert seen == [(1, 0, 0, 0), (0, 1, 1, 1), (1, 1, 1, 1), (0, 2, 2, 2)], seen
    all_captured = opt.flat.flat_p.detach().clone()
    # Trainer.zero_grad() after one micro-step restarts the window: the dropped micro-batch leaves no trace
    model, opt, tr, gs = _captured(2)
    _micro(gs, b[2])
    assert tr.accums == 1
    tr.zero_grad()
    assert tr.accums == 0
    for s in range(4):
        _micro(gs, b[s])
    torch.cuda.synchronize()
    assert tr.accums == 0 and int(tr.n_steps) == 2
    _assert_same_parameters(opt.flat.flat_p.detach(), all_captured, layout, 'restarted window vs fresh window')
    # an eager Trainer.step as micro-step 1 of 2 behind a captured micro-step 0 continues the window
    model, opt, tr, gs = _captured(2)
    _micro(gs, b[0])
    _eager_micro(tr, b[1])
    assert tr.accums == 0 and int(tr.n_steps) == 1
    _micro(gs, b[2]); _micro(gs, b[3])
    torch.cuda.synchronize()
    gs.check()
    assert tr.accums == 0 and int(tr.n_steps) == 2
    _assert_same_parameters(opt.flat.flat_p.detach(), all_captured, layout, 'eager micro-step 1 vs all captured')


# ---- 6. accum_iter == 1 is untouched -----------------------------------------------------------------------------------------------
def test_accum_iter_one_captures_what_it_always_did():
    model, opt, tr, gs = _captured(1)
    assert len(gs.graphs) == gs.n_seg == 1 and gs.opt_graph is None and gs.gate is None
    assert gs.kept_params > _n_linear(model) // 2
    li, la, gn = _micro(gs, _batch(64, 700))
    torch.cuda.synchronize()
    assert tr.accums == 0 and int(tr.n_steps) == 1 and np.isfinite(float(li) + float(la)) and float(gn) > 0
    from deepavfusion_amd.util.misc import GraphedStep
    model, opt, tr, cfg, O = _setup(1)
    gs = GraphedStep(tr, _batch(64, 700)[0].shape, _batch(64, 700)[1].shape)          # the default: noise drawn inside the graph
    assert not gs.inject_noise and gs.gate is None and gs.opt_graph is None
    with pytest.raises(ValueError):
        _micro(gs, _batch(64, 700))


# ---- fresh-process tests (last) ----------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.fresh_process
@pytest.mark.timeout(300)
def test_train_py_runs_captured_accumulation_and_resumes(tmp_path):
    """train.py at the sizes of test_train_py_runs_and_resumes with opt.accum_iter=2 opt.graph=True: the log names the captured
    accumulation mode and prints finite losses once per window; a second invocation resumes."""
    over = ['model.image.backbone=vit_tiny', 'model.audio.backbone=vit_tiny', 'model.fusion.num_heads=3', 'data.image_size=64',
            'data.audio_dur=2.', 'opt.batch_size=4', 'opt.epochs=2', 'opt.warmup_epochs=1', 'data.steps_per_epoch=4',
            'opt.accum_iter=2', 'opt.graph=True', 'log.print_freq=1', f'output_dir={tmp_path}', 'job_name=t', 'env.workers=0']
    import re
    for run in range(2):
        proc = subprocess.Popen([sys.executable, os.path.join(ROOT, 'train.py')] + over + (['opt.epochs=3'] if run else []),
                                cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
        try:
            out, _ = proc.communicate(timeout=130)
        finally:
            if proc.poll() is None:
                try:
                    os.killpg(proc.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                proc.wait(10)
        assert proc.returncode == 0, out[-4000:]
        assert 'captured step: accum_iter=2' in out, out[-4000:]
        lines = [l for l in out.splitlines() if '[Train]' in l]
        per_epoch = int(re.search(r' step \d+/(\d+) ', lines[0]).group(1)) // 2          # windows per epoch
        assert per_epoch >= 2 and len(lines) == per_epoch * (2 if run == 0 else 1), out[-4000:]      # one line per window
        for l in lines:
            assert int(re.search(r' step (\d+)/', l).group(1)) % 2 == 1, l               # printed on a window's last micro-step
            loss, norm = (float(re.search(rf' {k} ([0-9.eE+-]+|nan|inf)', l).group(1)) for k in ('loss', 'grad_norm'))
            assert np.isfinite(loss) and loss > 0 and np.isfinite(norm) and norm > 0, l
    ck = torch.load(os.path.join(str(tmp_path), 't', 'checkpoints', 'checkpoint_latest.pth'), map_location='cpu')
    assert ck['epoch'] == 3 and int(ck['n_steps']) == 3 * per_epoch           # resumed at epoch 2, ran one more epoch


@pytest.mark.fresh_process
@pytest.mark.timeout(240)
def test_captured_accumulation_over_one_rank_rccl(tmp_path):
    """DAV_FORCE_DIST=1, accum_iter = 2, captured (tests/accum_dp_worker.py, a fresh process in its own session, bounded, killed in a
    ``finally``): micro-step 0 launches no bucket, micro-step 1 launches every bucket exactly once, the parameters equal the
    non-distributed captured window (1e-3: graph_param_rel of test_dp_rccl_gpu.py), and it trains."""
    outdir, limit_s = str(tmp_path), 180
    env = dict(os.environ, DAV_WORKER_DUMP_S=str(limit_s - 20), PYTHONUNBUFFERED='1')
    proc = subprocess.Popen([sys.executable, WORKER, outdir, str(_free_port())], stdout=open(os.path.join(outdir, 'stdout0.txt'), 'w'),
                            stderr=subprocess.STDOUT, env=env, cwd=ROOT, start_new_session=True)
    try:
        deadline = time.time() + limit_s
        while time.time() < deadline and proc.poll() is None:
            time.sleep(0.25)
        code = proc.poll()
    finally:
        if proc.poll() is None:
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
            try:
                proc.wait(10)
            except subprocess.TimeoutExpired:
                pass
    diag = '\n'.join(f'--- {fn} ---\n' + open(os.path.join(outdir, fn), errors='replace').read()[-6000:]
                     for fn in sorted(os.listdir(outdir)) if fn.endswith(('.log', '.trace', '.txt')))
    assert code == 0, f'worker exit code {code}\n' + diag
    r = json.load(open(os.path.join(outdir, 'result0.json')))
    print(r)
    assert r['n_buckets'] >= 3 and r['segments'] >= 2 and r['sched_complete'], r
    for w in r['launches']:                                       # per window: [after micro-step 0, after micro-step 1]
        assert w[0] == [] and sorted(w[1]) == list(range(r['n_buckets'])), r
    assert r['accums'] == [1, 0] * len(r['launches']) and r['n_steps'] == len(r['launches']), r
    assert r['param_rel'] < 1e-3, r
    for a, b in zip(*r['losses']):
        assert abs(a - b) < 2e-3 * abs(a), r['losses']
    assert r['losses'][1][-1] < r['losses'][1][0], r['losses']    # it trains
