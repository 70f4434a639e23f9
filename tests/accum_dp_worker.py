"""Worker process of tests/test_accum_graph_gpu.py::test_captured_accumulation_over_one_rank_rccl (not collected by pytest).
Started as a FRESH python process in its own session; writes one line per phase to <outdir>/rank0.log, arms faulthandler so a
hang leaves a traceback, and always exits.

    python tests/accum_dp_worker.py <outdir> <port>        # 1-rank RCCL group on cuda:0 (DAV_FORCE_DIST=1)

Gradient accumulation (accum_iter = 2) in the captured step, once without and once with the data-parallel wrapper: the segmented
graphs are replayed per micro-batch, the bucket schedule runs on the window's last micro-step only (util/misc.py:144-148)."""
import datetime
import faulthandler
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUTDIR, PORT = sys.argv[1], sys.argv[2]
_LOG = open(os.path.join(OUTDIR, 'rank0.log'), 'w', buffering=1)
_TRACE = open(os.path.join(OUTDIR, 'rank0.trace'), 'w', buffering=1)
faulthandler.enable(file=_TRACE)
faulthandler.dump_traceback_later(int(os.environ.get('DAV_WORKER_DUMP_S', '150')), repeat=False, file=_TRACE, exit=True)
_T0 = time.time()


def phase(msg):
    _LOG.write(f'[{time.time() - _T0:7.2f}s] {msg}\n')


os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=PORT, RANK='0', WORLD_SIZE='1', HSA_ENABLE_IPC_MODE_LEGACY='0', DAV_FORCE_DIST='1')

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

WINDOWS = 3


def main():
    from deepavfusion_amd import engine
    from deepavfusion_amd.build_model import build_avmae
    from deepavfusion_amd.configs import CONFIGS
    from deepavfusion_amd.util import lr_sched
    from deepavfusion_amd.util.flat import FlatAdamW
    from deepavfusion_amd.util.misc import GraphedStep, Trainer
    from oracle import avmae_oracle as O
    from oracle.configs import CONFIGS as OC
    phase('init_process_group nccl')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, timeout=datetime.timedelta(seconds=60))
    phase('process group up')
    batches = []
    for s in range(2):
        image, audio, ni, na = O.synthetic_batch(OC['micro'], 64, seed=700 + s)
        batches.append((image.cuda(), audio.cuda(), torch.from_numpy(ni).cuda(), torch.from_numpy(na).cuda()))
    out, finals, losses = {}, [], []
    for distributed in (False, True):
        engine.set_grad_ready_hook(None)
        model = build_avmae(CONFIGS['micro']).cuda()
        model.load_state_dict(O.closed_form_state(OC['micro'], 0), strict=True)
        nd = [n for n, p in model.named_parameters() if 'bias' in n or 'norm' in n]
        groups = lr_sched.param_groups_pretrained(model, 0.05, no_weight_decay_list=nd, image_pt='', audio_pt='')
        opt = FlatAdamW(groups, lr=1e-3, betas=(0.9, 0.95), model=model)
        tr = Trainer(model, optimizer=opt, accum_iter=2, distributed=distributed, bucket_mb=0.5, first_bucket_mb=0.25)
        phase(f'capture distributed={distributed}')
        gs = GraphedStep(tr, batches[0][0].shape, batches[0][1].shape, inject_noise=True)
        if distributed:
            red = gs.reducer
            assert gs.dist_active and red.force and red.world == 1 and gs.opt_graph is not None
            sched = [bi for seg in gs.bucket_sched for bi in seg]
            out.update(n_buckets=len(red.buckets), segments=gs.n_seg, sched_complete=sorted(sched) == list(range(len(red.buckets))),
                       kept_params=gs.kept_params, launches=[], accums=[])
        else:
            assert gs.n_seg == 1 and gs.reducer is None
        run = []
        for w in range(WINDOWS):
            per_micro = []
            for m in range(2):
                b = batches[m]
                li, la, gn = gs(b[0], b[1], noise_image=b[2], noise_audio=b[3])
                run.append(float(li) + float(la))
                if distributed:
                    per_micro.append(list(red.launch_order))
                    out['accums'].append(tr.accums)
            if distributed:
                out['launches'].append(per_micro)
        torch.cuda.synchronize()
        gs.check()
        phase(f'replays done distributed={distributed}')
        if distributed:
            out['n_steps'] = int(tr.n_steps)
        losses.append(run)
        finals.append(opt.flat.flat_p.detach().clone())
    out['losses'] = losses
    out['param_rel'] = float((finals[1] - finals[0]).norm() / finals[0].norm())
    with open(os.path.join(OUTDIR, 'result0.json'), 'w') as f:
        json.dump(out, f)
    phase('result written')
    dist.destroy_process_group()
    phase('done')


if __name__ == '__main__':
    try:
        main()
    except BaseException as e:                                   # noqa: BLE001
        import traceback
        phase('FAILED ' + repr(e))
        traceback.print_exc(file=_TRACE)
        _TRACE.flush()
        os._exit(1)
    faulthandler.cancel_dump_traceback_later()
    os._exit(0)          # skip interpreter teardown: nothing after the results may hang this process
