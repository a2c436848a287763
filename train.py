"""Training entry point: the reference's loop (src/train.py, src/trainer.py:95-161) on the MI355X-native model.

    python train.py --config CFG [--logdir DIR] [--dev] [--name NAME] [--num_workers N] [--resume CKPT_OR_DIR]
                    [--batch B] [--steps K] [--validate_every V] [--seed S] [--freeze_backbone] [--accumulate K] [--gpus N]
                    [--skip_nonfinite]
                    [--synthetic N | --data_root ROOT --info TRAIN_INFO.pkl]

Every step: device-side training batch (regtr_amd.augment), RegTR.training_step, backward, the fused clip + AdamW step
(regtr_amd.optim.FusedAdamW, from RegTR.configure_optimizers) and StepLR.  Every --validate_every steps: validation_step over the
validation batches, validation_epoch_end, and a checkpoint `<log>/ckpt/model-<step>.pth` = {'state_dict', 'step', 'optimizer',
'scheduler'} with `<log>/ckpt/checkpoints.txt` (first line `Best step: N`), the reference's CheckPointManager layout.  --resume takes such
a file or folder and restores model, optimiser, scheduler and the global step; the batches continue at that step of the (seed, step)
sequence, so a resumed run computes what the unbroken one does.

--synthetic N: N seeded synthetic training items (3DMatch config: SyntheticPairs; ModelNet config: 2048-point clouds) and N // 4 (at
least 1) more for validation.  Real data: 3DMatch through --data_root / --info (the reference's train_info.pkl layout; validation then
needs --val_info); ModelNet HDF5 reading is not built (h5py is not a dependency): hand arrays to harness.modelnet_train_batches.
--accumulate K: an optimiser step averages the gradients of K micro-batches (regtr_amd.grad_bucket.GradBucket); --gpus N (1 .. 8): N
ranks, one per GPU, started as a child `python -m torch.distributed.run` job with a 127.0.0.1 rendezvous before this process touches a
GPU; every optimiser step then averages K x N micro-batches with ONE all-reduce, and a run with (K, N) averages the same micro-batches as
a run with (K x N, 1).  --steps and the checkpoints' step count optimiser steps.  A checkpoint written with K x N > 1 carries both
numbers, and --resume refuses another product.  Rank 0 alone logs and saves.
--skip_nonfinite (or `skip_nonfinite: true` in the config): an optimiser step whose gradient is not finite is left out on the device, and
with --accumulate / --gpus a micro-batch whose gradient is not finite is left out of the average on every rank alike
(FusedAdamW / GradBucket / train_loop with skip_nonfinite=True); the scheduler and the batch sequence go on.  The log line then shows both
counts, checkpoints carry them ('nonfinite_guard') and --resume restores them.
No tensorboard summaries.  Validation batches go through the same augmentation chain as training ones, at a fixed seed."""
import argparse
import logging
import os
import sys
import time

os.environ.setdefault('OMP_WAIT_POLICY', 'PASSIVE')      # idle OpenMP workers must not spin against a cgroup CPU quota

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

parser = argparse.ArgumentParser()
parser.add_argument('--config', type=str, help='Path to the config file.')
parser.add_argument('--logdir', type=str, default='../logs', help='Directory to store logs, summaries, checkpoints.')
parser.add_argument('--dev', action='store_true', help='If true, will ignore logdir and log to ../logdev instead')
parser.add_argument('--name', type=str, help='Prefix to add to logging directory')
parser.add_argument('--num_workers', type=int, default=-1, help='loader processes of the 3DMatch pair source (-1: 4; 0: one loader thread)')
parser.add_argument('--resume', type=str, help='Checkpoint file, or a folder with checkpoints.txt (its best step), to resume from')
parser.add_argument('--batch', type=int, default=0, help='items per training batch (default: cfg.train_batch_size, else 1)')
parser.add_argument('--synthetic', type=int, default=0, help='train on N seeded synthetic items instead of dataset files')
parser.add_argument('--data_root', type=str, default=None, help='overrides cfg.root (3DMatch)')
parser.add_argument('--info', type=str, default=None, help='3DMatch training info pickle')
parser.add_argument('--val_info', type=str, default=None, help='3DMatch validation info pickle')
parser.add_argument('--steps', type=int, default=100, help='training steps of this run (after --resume: further steps)')
parser.add_argument('--validate_every', type=int, default=0, help='validate and save a checkpoint every this many global steps (0: never)')
parser.add_argument('--seed', type=int, default=0, help='seed of the batch order and the augmentation draws')
parser.add_argument('--freeze_backbone', action='store_true', help='train only what sits above the KPConv backbone')
parser.add_argument('--log_every', type=int, default=50)
parser.add_argument('--accumulate', type=int, default=1, help='micro-batches whose gradients are averaged into one optimiser step')
parser.add_argument('--skip_nonfinite', action='store_true', help='leave non-finite optimiser steps and micro-batches out, on the device')
parser.add_argument('--gpus', type=int, default=0, help='N ranks, one per GPU (1 .. 8), as a child torch.distributed.run job; 0: this process alone')


def prepare_logger(opt, rank=0):
    """cvhelpers.misc.prepare_logger: <logdir>/<yymmdd_HHMMSS>[_name] (or ../logdev with --dev), log.txt inside (rank 0's only)."""
    if opt.dev:
        log_path = '../logdev'
    else:
        stamp = time.strftime('%y%m%d_%H%M%S')
        log_path = os.path.join(opt.logdir, stamp if not opt.name else f'{stamp}_{opt.name}')
    logger = logging.getLogger('regtr_amd.train')
    logger.setLevel(logging.INFO)
    handlers = [logging.StreamHandler()]
    if rank == 0:
        os.makedirs(log_path, exist_ok=True)
        handlers.append(logging.FileHandler(os.path.join(log_path, 'log.txt')))
    for h in handlers:
        h.setFormatter(logging.Formatter('%(asctime)s [%(levelname)s] %(message)s'))
        logger.addHandler(h)
    return logger, log_path


class _SyntheticClouds:
    """Indexable source of seeded raw ModelNet-like clouds (regtr_amd.synthetic.synth_modelnet_cloud)."""

    def __init__(self, n, first=0):
        self.n, self.first = n, first

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from regtr_amd.synthetic import synth_modelnet_cloud
        return synth_modelnet_cloud(self.first + i)


def launch_ranks(n):
    """--gpus N: this command line again as N ranks of a torch.distributed.run job, a CHILD process (this one has not touched a GPU and
    never does).  -> the job's exit code."""
    import socket
    import subprocess
    with socket.socket() as s_:
        s_.bind(('127.0.0.1', 0))
        port = s_.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    opt = parser.parse_args()
    if opt.accumulate < 1:
        sys.exit('--accumulate must be at least 1')
    if opt.gpus and not 1 <= opt.gpus <= 8:
        sys.exit('--gpus takes 1 .. 8')
    if opt.gpus and 'RANK' not in os.environ:
        sys.exit(launch_ranks(opt.gpus))
    rank, local_rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('LOCAL_RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    if not torch.cuda.is_available():
        sys.exit('regtr_amd runs on an MI355X (HIP) device only; there is no CPU path')
    if opt.config is None:
        if opt.resume is None or not os.path.exists(opt.resume):
            sys.exit('--config needs to be supplied unless resuming from checkpoint')
        folder = opt.resume if os.path.isdir(opt.resume) else os.path.dirname(opt.resume)
        opt.config = os.path.normpath(os.path.join(folder, '../config.yaml'))
        if not os.path.exists(opt.config):
            sys.exit('Config not found in resume directory')
    logger, log_path = prepare_logger(opt, rank)
    with open(opt.config, 'r') as fin:
        text = fin.read()
    if rank == 0 and os.path.abspath(opt.config) != os.path.abspath(os.path.join(log_path, 'config.yaml')):
        with open(os.path.join(log_path, 'config.yaml'), 'w') as fout:
            fout.write(f'# Original file name: {opt.config}\n' + text)

    from regtr_amd import RegTR, harness, load_config
    torch.set_num_threads(max(1, min(torch.get_num_threads(), harness.usable_cores() // 2, 8)))
    cfg = load_config(opt.config)
    device = torch.device('cuda', local_rank)
    batch = opt.batch if opt.batch > 0 else int(cfg.get('train_batch_size', 1))
    modelnet = cfg.dataset == 'modelnet'
    workers = opt.num_workers if opt.num_workers >= 0 else 4

    # sources
    if opt.synthetic > 0:
        n_val = max(1, opt.synthetic // 4)
        if modelnet:
            source, val_source = _SyntheticClouds(opt.synthetic), _SyntheticClouds(n_val, first=1 << 20)
        else:
            source, val_source = harness.SyntheticPairs(opt.synthetic), harness.SyntheticPairs(n_val, pairs_per_scene=1)
    elif modelnet:
        logger.error('ModelNet HDF5 reading is not built (h5py is not a dependency); use --synthetic N or harness.modelnet_train_batches')
        sys.exit(-4)
    else:
        cfg_root = cfg.get('root', None)
        roots = [opt.data_root] if opt.data_root else ([cfg_root] if isinstance(cfg_root, str) else list(cfg_root or []))
        root = next((r for r in roots if os.path.exists(r)), None)
        if root is None or not opt.info or not os.path.exists(opt.info):
            logger.error(f'Dataset not found (info {opt.info}, roots {roots}); pass --data_root and --info, or use --synthetic N')
            sys.exit(-4)
        source = harness.ThreeDMatchPairs(opt.info, root)
        val_source = harness.ThreeDMatchPairs(opt.val_info, root) if opt.val_info else None

    # loader processes of the pair source: forked before this process holds a HIP context (as test.py)
    pool = None
    if not modelnet and workers > 0:
        import atexit
        pool = harness.LoaderPool(None, device, workers=workers, max_batch=batch)
        atexit.register(pool.close)
    torch.cuda.set_device(device)
    if pool is not None:
        pool.set_source(source)
        pool.prepare()
    if 'RANK' in os.environ:             # under torch.distributed.run: a process group at every world size (one code path)
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group('nccl', device_id=device)

    torch.manual_seed(opt.seed)          # the initial weights (and numpy: the kernel points' random rotation) follow --seed, as setup_seed
    np.random.seed(opt.seed % (1 << 32))
    if opt.skip_nonfinite:
        cfg['skip_nonfinite'] = True
    guarded = bool(cfg.get('skip_nonfinite', False))
    model = RegTR(cfg).to(device)
    model.configure_optimizers(train_backbone=not opt.freeze_backbone)
    first_step, counters = 0, None
    k, group = opt.accumulate, opt.accumulate * world
    if opt.resume:
        ck, cw = harness.CheckpointSaver.batching(opt.resume)
        if ck * cw != group:
            logger.error(f'--resume: {opt.resume} was written with accumulate x world = {ck} x {cw} = {ck * cw}, this run has '
                         f'{k} x {world} = {group}; an optimiser step must average the same number of micro-batches')
            sys.exit(-5)
        first_step = harness.CheckpointSaver.load(opt.resume, model, map_location=device, optimizer=model.optimizer, scheduler=model.scheduler)
        counters = harness.CheckpointSaver.counters(opt.resume) if guarded else None
        logger.info(f'Resumed from {opt.resume} at step {first_step}')

    per_epoch = -(-len(source) // batch)
    epochs = -(-(first_step + opt.steps) * group // per_epoch)      # (micro-batches: an optimiser step consumes `group` of them)
    share = dict(first_step=first_step * group, accumulate=k, rank=rank, world=world)
    if modelnet:
        batches = harness.modelnet_train_batches(source, cfg, batch, opt.seed, epochs=epochs, device=device, **share)
        val_batches = lambda: harness.modelnet_train_batches(val_source, cfg, batch, opt.seed + 1, epochs=1, device=device)
    else:
        batches = harness.train_batches(source, cfg, batch, opt.seed, epochs=epochs, device=device, num_workers=workers, loader_pool=pool,
                                        **share)
        val_batches = (lambda: harness.train_batches(val_source, cfg, batch, opt.seed + 1, epochs=1, device=device, num_workers=0)) \
            if val_source is not None else None
    saver = harness.CheckpointSaver(os.path.join(log_path, 'ckpt')) if opt.validate_every > 0 and rank == 0 else None
    t0 = time.perf_counter()
    out = harness.train_loop(model, batches, opt.steps, first_step=first_step, train_backbone=not opt.freeze_backbone,
                             validate_every=opt.validate_every, val_batches=val_batches, saver=saver, logger=logger, log_every=opt.log_every,
                             accumulate=k, **(dict(skip_nonfinite=True, counters=counters) if guarded else {}))
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    avg = ', '.join(f'{k} {float(v):.4g}' for k, v in out['loss_avg'].items())
    if rank == 0:
        logger.info(f'Ending training. Number of training steps = {out["step"]} ({out["step"] - first_step} in {dt:.1f} s); average losses: {avg}')
    if 'RANK' in os.environ:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
