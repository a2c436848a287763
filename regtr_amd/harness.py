"""Batched, streamed inference harness: what test.py / demo.py run around `RegTR.forward`.

Replaces, for inference only, the reference's Trainer.test loop (/root/reference/src/trainer.py:177-211) and
GenericRegModel.test_step / _save_3DMatch_log (models/generic_reg_model.py:130-158, 260-281):
  * B pairs per forward instead of one (conf test_batch_size: 1), next batch loaded by a worker thread into pinned
    memory and copied to the GPU on a side stream while the current batch computes;
  * no tensorboard, no per-pair host synchronisation: poses stay on the device until the end of the set;
  * optionally (losses=True, test.py --losses) the reference's test losses: RegTR.compute_loss per pair on GT masks from
    overlap.compute_overlap_masks, kept on the device and reduced once at the end (the `[Losses]` line of test_epoch_end);
  * pairs sharded over ranks (one process per GPU) with a single RCCL gather of the poses; rank 0 writes the logs;
  * `est.log` blocks / `pred_transforms.npy` in the reference's exact formats, so the reference's own evaluation scripts
    (benchmark_predator / RPMNet eval) read them unchanged.
"""
import json
import os
import pickle
import queue
import threading
import time

import numpy as np
import torch

from .distributed import gather_poses, shard_pairs


def usable_cores():
    """Host cores this process may actually use: the affinity mask capped by a cgroup CPU quota (os.cpu_count() reports the machine's
    cores even inside a quota-limited container; thread teams larger than the quota spin against each other until the kernel throttles
    the whole process)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()
        if quota != 'max':
            n = min(n, max(1, int(float(quota) / float(period))))
    except (OSError, ValueError):
        pass
    try:
        q = int(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
        per = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
        if q > 0:
            n = min(n, max(1, q // per))
    except (OSError, ValueError):
        pass
    return n


# ------------------------------------------------------------------------------------------------------ point cloud files
def read_ply_xyz(fname):
    """Minimal PLY reader (ascii / binary_little_endian, vertex x y z as float or double) -- stands in for
    open3d.io.read_point_cloud in demo.py:145-147."""
    with open(fname, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise AssertionError(f'{fname}: not a PLY file')
        fmt, n_vert, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise AssertionError(f'{fname}: truncated PLY header')
            tok = line.split()
            if not tok:
                continue
            if tok[0] == b'format':
                fmt = tok[1].decode()
            elif tok[0] == b'element':
                in_vertex = tok[1] == b'vertex'
                if in_vertex:
                    n_vert = int(tok[2])
            elif tok[0] == b'property' and in_vertex:
                props.append((tok[1].decode(), tok[2].decode()))
            elif tok[0] == b'end_header':
                break
        names = [p[1] for p in props]
        if not all(a in names for a in 'xyz'):
            raise AssertionError(f'{fname}: vertex element has no x/y/z')
        if fmt == 'ascii':
            rows = np.loadtxt(f, max_rows=n_vert, ndmin=2)
            return rows[:, [names.index(a) for a in 'xyz']].astype(np.float64)
        if fmt != 'binary_little_endian':
            raise AssertionError(f'{fname}: unsupported PLY format {fmt}')
        np_t = {'float': '<f4', 'float32': '<f4', 'double': '<f8', 'float64': '<f8', 'uchar': 'u1', 'uint8': 'u1', 'char': 'i1',
                'int8': 'i1', 'short': '<i2', 'int16': '<i2', 'ushort': '<u2', 'uint16': '<u2', 'int': '<i4', 'int32': '<i4',
                'uint': '<u4', 'uint32': '<u4'}
        dt = np.dtype([(n, np_t[t]) for t, n in props])
        data = np.frombuffer(f.read(n_vert * dt.itemsize), dtype=dt, count=n_vert)
        return np.stack([data['x'], data['y'], data['z']], 1).astype(np.float64)


def load_point_cloud(fname, cache_dir=None):
    """demo.py:142-153: .pth (torch-saved array), .ply, .bin (KITTI float32 x y z r), and .npy (a plain array); returns (N, 3).
    cache_dir: `.pth` fragments (a zip + pickle: ~2 ms each to open, 3562 of them in the 3DLoMatch list) are mirrored there once as
    float32 `.npy` files and read back with np.load (~0.1 ms); a cache entry older than its source is rebuilt."""
    if cache_dir is not None and fname.endswith('.pth'):
        cname = os.path.join(cache_dir, os.path.abspath(fname).strip(os.sep).replace(os.sep, '__')[:-4] + '.npy')
        try:
            if os.path.getmtime(cname) >= os.path.getmtime(fname):
                return np.load(cname)
        except OSError:
            pass
        data = np.ascontiguousarray(load_point_cloud(fname), dtype=np.float32)
        os.makedirs(cache_dir, exist_ok=True)
        tmp = f'{cname}.{os.getpid()}.tmp.npy'
        np.save(tmp, data)
        os.replace(tmp, cname)                       # atomic: concurrent loader processes may race for the same entry
        return data
    if fname.endswith('.pth'):
        data = torch.load(fname, weights_only=False)
        data = data.numpy() if isinstance(data, torch.Tensor) else np.asarray(data)
    elif fname.endswith('.ply'):
        data = read_ply_xyz(fname)
    elif fname.endswith('.bin'):
        data = np.fromfile(fname, dtype=np.float32).reshape(-1, 4)
    elif fname.endswith('.npy'):
        data = np.load(fname)
    else:
        raise AssertionError('Cannot recognize point cloud format')
    return data[:, :3]


# ------------------------------------------------------------------------------------------------------ pair sources
class ThreeDMatchPairs:
    """The 3DMatch / 3DLoMatch test pairs (data_loaders/threedmatch.py:20-101, test phase): an info pickle with keys
    rot (3,3), trans (3,1), src, tgt (paths relative to `root`), overlap."""

    def __init__(self, info_fname, root, cache_dir=None):
        with open(info_fname, 'rb') as fid:
            self.infos = pickle.load(fid)
        self.root, self.cache_dir = root, cache_dir

    def __len__(self):
        return len(self.infos['rot'])

    def __getitem__(self, i):
        src_path, tgt_path = self.infos['src'][i], self.infos['tgt'][i]
        pose = np.concatenate([self.infos['rot'][i], self.infos['trans'][i].reshape(3, 1)], 1).astype(np.float32)
        return {'src_xyz': np.ascontiguousarray(load_point_cloud(os.path.join(self.root, src_path), self.cache_dir), dtype=np.float32),
                'tgt_xyz': np.ascontiguousarray(load_point_cloud(os.path.join(self.root, tgt_path), self.cache_dir), dtype=np.float32),
                'pose': pose, 'idx': i, 'src_path': src_path, 'tgt_path': tgt_path}

    # the fragment protocol of run_test_shared: a pair names its two fragments, a fragment is loaded by its name
    def fragment_keys(self, i):
        """(src_key, tgt_key) of pair i: the fragments' paths relative to `root`."""
        return self.infos['src'][i], self.infos['tgt'][i]

    def load_fragment(self, key):
        """The (n, 3) float32 cloud of fragment `key` (through load_point_cloud and its .npy cache)."""
        return np.ascontiguousarray(load_point_cloud(os.path.join(self.root, key), self.cache_dir), dtype=np.float32)


class SyntheticPairs:
    """N deterministic synthetic 3DMatch-sized pairs (regtr_amd/synthetic.py) laid out like the 3DMatch test set
    (scene folders, cloud_bin_<k>.pth names) so that the est.log writer is exercised unchanged."""

    def __init__(self, n, points=20000, pairs_per_scene=64, overlap=None):
        self.n, self.points, self.pps, self.overlap = n, points, pairs_per_scene, overlap

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from .synthetic import synth_pair
        src, tgt, pose = synth_pair(i, self.points, return_pose=True, overlap=self.overlap)
        sp, tp = _synthetic_paths(self, i)
        return {'src_xyz': src, 'tgt_xyz': tgt, 'pose': pose, 'idx': i, 'src_path': sp, 'tgt_path': tp}


def _materialize_one(args):
    root, n, points, overlap, distinct, i = args
    src = SyntheticPairs(n, points, overlap=overlap)
    it = src[i % distinct if distinct else i]
    for rel, arr in zip(_synthetic_paths(src, i), (it['src_xyz'], it['tgt_xyz'])):
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        torch.save(arr, os.path.join(root, rel))
    return i, it['pose']


def materialize_synthetic(root, n, points=20000, overlap=None, logger=None, rank=0, world=1, distinct=0, procs=None):
    """Writes N synthetic pairs in the layout of the 3DMatch test set -- <root>/test/<scene>/cloud_bin_<k>.pth (torch-saved (N,3) float32
    arrays, what data_loaders/threedmatch.py:74-75 torch.load()s) and an info pickle (keys rot, trans, src, tgt, overlap,
    threedmatch.py:34-40) -- so that ThreeDMatchPairs, the loader thread and the est.log writer run exactly as on the real data set.
    Rank r generates and writes pairs r, r + world, ...; the ground-truth poses are exchanged through small per-rank files, so the
    pickle is complete on every rank.  distinct > 0: only that many different pairs are generated (pair i = pair i % distinct; every pair still
    gets its own two files, so the loader's work is the full set's) -- set-up time of the end-to-end measurement.  The pairs are generated
    by `procs` processes (default: the usable cores, at most 16; spawned, so the caller may already hold a GPU).  -> info pickle path"""
    src = SyntheticPairs(n, points, overlap=overlap)
    t0 = time.perf_counter()
    os.makedirs(root, exist_ok=True)
    path = os.path.join(root, f'test_info.rank{rank}.pkl')
    stamp = os.path.join(root, f'complete.rank{rank}.json')           # written last: (n, points, overlap, world) of a finished set
    want = json.dumps([n, points, overlap, world, distinct])
    if world == 1 and os.path.exists(stamp) and open(stamp).read() == want and os.path.exists(path):
        if logger:
            logger.info(f'{n} synthetic pairs already materialised under {root}')
        return path
    poses = {}
    todo = [(root, n, points, overlap, distinct, i) for i in range(rank, n, world)]
    procs = procs if procs is not None else max(1, min(16, len(os.sched_getaffinity(0)) // max(world, 1)))
    if procs > 1 and len(todo) >= 32:        # (spawned workers import torch: seconds each -- not worth it for a handful of pairs)
        import multiprocessing as mp
        with mp.get_context('spawn').Pool(procs) as pool:
            for i, pose in pool.imap_unordered(_materialize_one, todo, chunksize=max(1, len(todo) // (8 * procs))):
                poses[i] = pose
    else:
        for a in todo:
            i, pose = _materialize_one(a)
            poses[i] = pose
    with open(os.path.join(root, f'poses.rank{rank}.pkl'), 'wb') as f:
        pickle.dump(poses, f)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()                      # every rank's files exist before anyone reads
    for r in range(world):
        if r != rank:
            with open(os.path.join(root, f'poses.rank{r}.pkl'), 'rb') as f:
                poses.update(pickle.load(f))
    infos = {'rot': [], 'trans': [], 'src': [], 'tgt': [], 'overlap': []}
    for i in range(n):
        sp, tp = _synthetic_paths(src, i)
        infos['rot'].append(poses[i][:, :3].astype(np.float64)); infos['trans'].append(poses[i][:, 3:].astype(np.float64))
        infos['src'].append(sp); infos['tgt'].append(tp); infos['overlap'].append(0.0)
    with open(path, 'wb') as f:
        pickle.dump(infos, f)
    with open(stamp, 'w') as f:
        f.write(want)
    if logger:
        logger.info(f'{n} synthetic pairs materialised under {root} in {time.perf_counter() - t0:.1f} s')
    return path


def _synthetic_paths(src, i):
    scene, k = i // src.pps, i % src.pps
    return (f'test/synthetic-scene{scene:03d}/cloud_bin_{2 * k + 1}.pth', f'test/synthetic-scene{scene:03d}/cloud_bin_{2 * k}.pth')


class SyntheticScenePairs:
    """Scene-style synthetic pairs: n_scenes rooms of fragments_per_scene fragments each (regtr_amd.synthetic.synth_fragments: occluded,
    rigidly moved views of ONE room) and pairs_per_scene pairs of them per room -- the shape of the 3DMatch test lists, where a few hundred
    fragments make 1623 / 1781 pairs.  A scene's pairs are its (a, b), a < b, in lexicographic order, then the same reversed, cyclically; pair
    i is pair i // n_scenes of scene i % n_scenes (consecutive pairs come from different scenes: the order that is hardest on a small
    bank).  Laid out like the 3DMatch test set (scene folders, cloud_bin_<k>.pth names) so that the est.log writer is exercised unchanged.
    Serves both protocols: pairs[i] (a plain pair, what run_test and the LoaderPool processes read; the source pickles) and
    fragment_keys / load_fragment (run_test_shared).  meta(i) gives a pair's paths and ground-truth pose without generating a cloud.
    cache_scenes: generated scenes kept (least recently used dropped; a scene is F clouds of `points` points); since consecutive pairs
    walk the scenes, it should cover the scenes one window of pairs touches -- default min(n_scenes, 64)."""

    _PREFIX = 'synthetic-scene'

    def __init__(self, n_scenes, fragments_per_scene, pairs_per_scene, points=20000, cache_scenes=None):
        if n_scenes < 1 or fragments_per_scene < 2 or pairs_per_scene < 1:
            raise ValueError('SyntheticScenePairs: at least one scene, two fragments per scene and one pair per scene')
        self.n_scenes, self.fps, self.pps, self.points = n_scenes, fragments_per_scene, pairs_per_scene, points
        self.cache_scenes = max(1, min(n_scenes, 64) if cache_scenes is None else int(cache_scenes))
        F = fragments_per_scene
        fwd = [(a, b) for a in range(F) for b in range(a + 1, F)]
        self._scene_pairs = fwd + [(b, a) for a, b in fwd]
        self._scenes, self._lock = {}, threading.Lock()

    def __getstate__(self):                   # (LoaderPool.set_source pickles the source: neither the lock nor the generated scenes travel)
        state = dict(self.__dict__)
        del state['_scenes'], state['_lock']
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._scenes, self._lock = {}, threading.Lock()

    def __len__(self):
        return self.n_scenes * self.pps

    def _scene(self, s):
        """The clouds of scene s, generated on first use."""
        with self._lock:                      # (the loader thread and the consumer may both ask)
            ent = self._scenes.pop(s, None)
            if ent is None:
                from .synthetic import synth_fragments
                while len(self._scenes) >= self.cache_scenes:
                    self._scenes.pop(next(iter(self._scenes)))       # the least recently used: hits are re-inserted at the end
                ent = synth_fragments(s, self.fps, self.points)[0]
            self._scenes[s] = ent
            return ent

    def _pair(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        s, k = i % self.n_scenes, i // self.n_scenes
        a, b = self._scene_pairs[k % len(self._scene_pairs)]
        return s, a, b

    @classmethod
    def _key(cls, s, k):
        return f'test/{cls._PREFIX}{s:03d}/cloud_bin_{k}.pth'

    def fragment_keys(self, i):
        s, a, b = self._pair(i)
        return self._key(s, a), self._key(s, b)

    def load_fragment(self, key):
        scene, name = key.split('/')[1:3]
        if not scene.startswith(self._PREFIX):
            raise KeyError(key)
        s, k = int(scene[len(self._PREFIX):]), int(name[:-4].split('_')[-1])
        if not (0 <= s < self.n_scenes and 0 <= k < self.fps):
            raise KeyError(key)
        return self._scene(s)[k]

    def pose(self, i):
        """The ground-truth (3, 4) float32 transform taking pair i's source into its target's frame (no cloud is generated)."""
        from .synthetic import synth_fragment_poses
        s, a, b = self._pair(i)
        return synth_fragment_poses(s, self.fps)[1][a, b, :3].astype(np.float32)

    def meta(self, i):
        """Pair i without its clouds: {'src_path', 'tgt_path', 'pose', 'idx'}."""
        sk, tk = self.fragment_keys(i)
        return {'pose': self.pose(i), 'idx': i, 'src_path': sk, 'tgt_path': tk}

    def __getitem__(self, i):
        item = self.meta(i)
        item['src_xyz'], item['tgt_xyz'] = self.load_fragment(item['src_path']), self.load_fragment(item['tgt_path'])
        return item


# ------------------------------------------------------------------------------------------------------ streaming
class Prefetcher:
    """Iterates `indices` of `pairs` in batches of `batch`; a worker thread loads the next batches (disk / generator,
    pinned host buffers), the H2D copies run on a side stream, and the consumer stream waits on an event only."""

    def __init__(self, pairs, indices, batch, device, depth=2):
        self.pairs, self.indices, self.batch, self.device = pairs, list(indices), batch, device
        self.q = queue.Queue(maxsize=depth)
        self.copy_stream = torch.cuda.Stream(device=device, priority=-1) if device.type == 'cuda' else None      # (own hardware-queue pool, see LoaderPool.iterate)
        self.thread = threading.Thread(target=self._work, daemon=True)
        self.thread.start()

    def _work(self):
        try:
            for s in range(0, len(self.indices), self.batch):
                items = [self.pairs[i] for i in self.indices[s:s + self.batch]]
                out = {'items': items}
                if self.copy_stream is not None:
                    with torch.cuda.stream(self.copy_stream):
                        for key in ('src_xyz', 'tgt_xyz'):
                            out[key] = [torch.from_numpy(it[key]).pin_memory().to(self.device, non_blocking=True) for it in items]
                        out['ready'] = torch.cuda.Event()
                        out['ready'].record(self.copy_stream)
                else:
                    for key in ('src_xyz', 'tgt_xyz'):
                        out[key] = [torch.from_numpy(it[key]) for it in items]
                self.q.put(out)
            self.q.put(None)
        except BaseException as e:      # surface loader errors in the consumer
            self.q.put(e)

    def __iter__(self):
        while True:
            b = self.q.get()
            if b is None:
                return
            if isinstance(b, BaseException):
                raise b
            if 'ready' in b:
                torch.cuda.current_stream(self.device).wait_event(b['ready'])
                for key in ('src_xyz', 'tgt_xyz'):      # the tensors were allocated on the copy stream
                    for t in b[key]:
                        t.record_stream(torch.cuda.current_stream(self.device))
            yield b


# ------------------------------------------------------------------------------------------------------ process-pool loading
# The reference feeds its test loop from a torch DataLoader with `--num_workers` processes (test.py:26, data_loaders/__init__.py:11-58),
# one pair per step.  Here a forward takes 64 pairs in ~27 ms, i.e. the loader has to deliver ~2300 pairs/s = 4600 files/s, and a
# torch-saved fragment takes ~2 ms to open: one Python thread (Prefetcher) tops out at ~450-530 pairs/s.  LoaderPool therefore
#   * runs `workers` loader PROCESSES (forked once, reusable over any number of passes; they inherit the pair source and never touch
#     the GPU), each assembling WHOLE batches;
#   * gives every in-flight batch one slab of shared memory (anonymous shared mappings: no page is touched until a worker fills it)
#     into which the worker writes the batch's clouds back to back in the forward's own order [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}]
#     -- no array is pickled through a pipe;
#   * moves a filled slab through one of two page-locked staging buffers to the GPU as ONE asynchronous copy on a side stream instead of
#     128 small ones, and hands the consumer per-cloud VIEWS of that one device buffer; the consumer stream waits on the copy's event.
# Measured on the 16-core-quota GPU boxes (profiles/r04_*_e2e_harness.txt): more than ~6 loader processes slow the set down (they compete
# with the launching thread for the quota), hence the default of 4.
_POOL_SLABS = {}             # pool id -> [numpy views of the pool's shared slabs]; set before the fork and kept until close(), so that a
#                              worker multiprocessing.Pool re-spawns later (forked from the parent THEN) finds them too
_POOL_SOURCES = {}           # (worker side) source file -> unpickled pair source, loaded once per worker
_PINNED = {}                 # (device, points) -> two page-locked staging buffers, kept for the life of the process
_POOL_IDS = [0]


def _pool_fill(task):
    """Runs in a loader process: loads the pairs `idxs` (one PART of a batch) and packs them into its region [lo, lo + cap) of slab
    `slab_id` as [src clouds ..., tgt clouds ...].  -> (b, part, lens_src, lens_tgt, ids, None) or, when the part does not fit its
    region, (b, part, None, None, ids, (src arrays, tgt arrays)) with the clouds pickled back (correct, slower).  Last element: the
    pairs' GT poses (3, 4) (None where the source has none), which RegTR.compute_loss needs (run_test(losses=True))."""
    b, part, idxs, slab_id, lo, cap, pool_id, source_file = task
    source = _POOL_SOURCES.get(source_file)
    if source is None:        # first task of this worker (or of a re-spawned one): the pair source arrives by file, not by fork
        import pickle
        with open(source_file, 'rb') as f:
            source = pickle.load(f)
        _POOL_SOURCES.clear()
        _POOL_SOURCES[source_file] = source
    items = [source[i] for i in idxs]
    src, tgt = [it['src_xyz'] for it in items], [it['tgt_xyz'] for it in items]
    ls, lt = [int(c.shape[0]) for c in src], [int(c.shape[0]) for c in tgt]
    ids = [int(it['idx']) for it in items]
    poses = [np.asarray(it['pose'], dtype=np.float32)[:3] if 'pose' in it else None for it in items]       # (GT poses: 48 B per pair)
    if sum(ls) + sum(lt) > cap:
        return b, part, None, None, ids, ([np.ascontiguousarray(c, dtype=np.float32) for c in src], [np.ascontiguousarray(c, dtype=np.float32) for c in tgt]), poses
    slab = _POOL_SLABS[pool_id][slab_id]
    o = lo
    for c, n in zip(src + tgt, ls + lt):
        slab[o:o + n] = c
        o += n
    return b, part, ls, lt, ids, None, poses


def _unlink_quiet(path):
    try:
        os.unlink(path)
    except OSError:
        pass


class LoaderPool:
    """`workers` forked loader processes + their shared slabs over one pair source; `iterate(indices, batch)` yields batches
    {'src_xyz': [...], 'tgt_xyz': [...], 'ids': [...]} of device tensors (CPU tensors for a cpu `device`: the tests' path), in order.
    The pool outlives a pass: create it once, iterate as often as needed, close() at the end.  It can (and test.py does) be created
    BEFORE the GPU is initialised and before torch.distributed -- forking a process that holds a HIP context / a process group copies that
    state into every worker: the constructor touches no GPU API, the pair source may be handed over later (`set_source`, by a pickle file:
    workers -- including ones multiprocessing re-spawns -- load it on their first task) and the page-locked staging buffers are made by
    `prepare()` / the first pass.  slab_points: capacity of a slab in points (default 1.25 x max_batch x 2 x 24k; a batch that does not
    fit comes back pickled -- correct, slower)."""

    def __init__(self, pairs, device, workers=4, max_batch=64, depth=None, slab_points=None, maxtasksperchild=None):
        import mmap
        import multiprocessing as mp
        self.device = torch.device(device)
        self.workers = max(1, int(workers))
        self.cuda = self.device.type == 'cuda'
        self.cap = int(slab_points or 1.25 * max_batch * 2 * 24000)
        n_slabs = depth or (self.workers + 2)
        self._maps = [mmap.mmap(-1, self.cap * 12) for _ in range(n_slabs)]           # MAP_SHARED | MAP_ANONYMOUS: inherited by the fork
        self.slabs = [np.frombuffer(m, dtype=np.float32).reshape(self.cap, 3) for m in self._maps]
        _POOL_IDS[0] += 1
        self.pool_id = _POOL_IDS[0]
        _POOL_SLABS[self.pool_id] = self.slabs          # stays registered until close(): re-spawned workers inherit it as well
        self.pool = mp.get_context('fork').Pool(self.workers, maxtasksperchild=maxtasksperchild)
        self._source_file = None
        self.copy_stream = None
        self.last_timing = None
        if pairs is not None:
            self.set_source(pairs)
        if self.cuda and torch.cuda.is_initialized():
            self.prepare()

    def set_source(self, pairs):
        """The pair source the workers index (`pairs[i]` -> {'src_xyz', 'tgt_xyz', 'idx', ...}); must pickle."""
        import pickle
        import tempfile
        import weakref
        self._drop_source_file()
        fd, self._source_file = tempfile.mkstemp(prefix='regtr_pairs_', suffix='.pkl')
        with os.fdopen(fd, 'wb') as f:
            pickle.dump(pairs, f, protocol=pickle.HIGHEST_PROTOCOL)
        # sys.exit() / an exception / an abandoned pool: the file is removed when the pool is collected or the interpreter exits
        self._source_finalizer = weakref.finalize(self, _unlink_quiet, self._source_file)

    def _drop_source_file(self):
        if self._source_file is not None:
            fin = getattr(self, '_source_finalizer', None)
            if fin is not None:
                fin.detach()
            _unlink_quiet(self._source_file)
            self._source_file = None

    def prepare(self):
        """Page-locks the two staging buffers (tens of ms: not inside the first timed pass).  Needs the GPU runtime, so call it after
        torch.cuda.set_device when the pool was created before."""
        if self.cuda:
            self._staging()

    def _staging(self):
        key = (str(self.device), self.cap)
        if key not in _PINNED:
            _PINNED[key] = [torch.empty((self.cap, 3), dtype=torch.float32).pin_memory() for _ in range(2)]
        return _PINNED[key]

    def iterate(self, indices, batch):
        indices, batch = list(indices), int(batch)
        n_batches = (len(indices) + batch - 1) // batch
        free, pending, out = queue.Queue(), queue.Queue(), queue.Queue(maxsize=len(self.slabs))
        for sid in range(len(self.slabs)):
            free.put(sid)
        if self.cuda and self.copy_stream is None:
            # high priority = a hardware queue from another pool than the forward's stream (regtr.py: _side_stream; an RCCL communicator in
            # the process had put a normal-priority side stream onto the main stream's queue, i.e. behind the forward it should run next to)
            self.copy_stream = torch.cuda.Stream(device=self.device, priority=-1)
        if self._source_file is None:
            raise RuntimeError('LoaderPool.iterate: no pair source (set_source)')
        import sys
        interval = sys.getswitchinterval()
        if interval > 0.0005:
            sys.setswitchinterval(0.0005)    # the launching thread shares the interpreter with the two loader threads below: short GIL
        #                                      hand-offs for the duration of the pass (restored when the generator finishes)
        stage = self._staging() if self.cuda else None
        timing = {'wait_worker_s': 0.0, 'stage_copy_s': 0.0, 'h2d_wait_s': 0.0, 'batches': n_batches}
        self.last_timing = timing

        # a batch is loaded by up to `workers` processes at once: part p fills region p of the batch's slab (regions of equal capacity;
        # the copy into the staging buffer compacts them into the forward's order) -- the latency of the FIRST batch is what a short
        # set pays in full
        parts = max(1, min(self.workers, 8, batch // 8))
        region = self.cap // parts

        def dispatch():
            try:
                for b in range(n_batches):
                    sid = free.get()
                    idxs = indices[b * batch:(b + 1) * batch]
                    per = (len(idxs) + parts - 1) // parts
                    tasks = [(b, p, idxs[p * per:(p + 1) * per], sid, p * region, region, self.pool_id, self._source_file)
                             for p in range(parts) if idxs[p * per:(p + 1) * per]]
                    pending.put((sid, [self.pool.apply_async(_pool_fill, (t,)) for t in tasks]))
                pending.put(None)
            except BaseException as e:      # noqa: BLE001
                pending.put(e)

        def upload():
            try:
                staged = [None, None]                       # event behind the last H2D copy out of each staging buffer
                k = 0
                while True:
                    res = pending.get()
                    if res is None:
                        break
                    if isinstance(res, BaseException):
                        raise res
                    t0 = time.perf_counter()
                    sid, asyncs = res
                    done = [a.get() for a in asyncs]                # parts in order
                    t1 = time.perf_counter()
                    timing['wait_worker_s'] += t1 - t0
                    # pieces in the forward's order: every part's src clouds, then every part's tgt clouds
                    pieces, lens_s, lens_t, ids, gt = [[], []], [], [], [], []
                    for (b, part, ls, lt, pid, arrays, pp), t in zip(done, [a_ for a_ in range(len(done))]):
                        ids += pid
                        gt += pp
                        if arrays is not None:              # oversize part: the clouds came back by value
                            ls, lt = [int(a.shape[0]) for a in arrays[0]], [int(a.shape[0]) for a in arrays[1]]
                            pieces[0] += [torch.from_numpy(a) for a in arrays[0]]
                            pieces[1] += [torch.from_numpy(a) for a in arrays[1]]
                        else:
                            lo = part * region
                            pieces[0].append(torch.from_numpy(self.slabs[sid][lo:lo + sum(ls)]))
                            pieces[1].append(torch.from_numpy(self.slabs[sid][lo + sum(ls):lo + sum(ls) + sum(lt)]))
                        lens_s += ls; lens_t += lt
                    lens = lens_s + lens_t
                    n = sum(lens)
                    B = len(ids)
                    off = np.concatenate([[0], np.cumsum(lens)])
                    item = {'ids': ids, 'gt_pose': gt}
                    if self.cuda:
                        if n <= self.cap:
                            if staged[k] is not None:
                                staged[k].synchronize()     # this staging buffer's previous copy has left
                            pin = stage[k][:n]
                        else:
                            pin = torch.empty((n, 3), dtype=torch.float32).pin_memory()
                        # plain memcpy (numpy): a torch copy_ of this size wakes the whole intra-op thread team -- on a many-core host
                        # under a cgroup CPU quota the spinning team exhausts the quota and the kernel throttles EVERY thread of the
                        # process for the rest of the 100 ms period (40-70 ms stalls of the launching thread were measured that way)
                        pin_np = pin.numpy()
                        o = 0
                        for pc in pieces[0] + pieces[1]:
                            np.copyto(pin_np[o:o + pc.shape[0]], pc.numpy())
                            o += pc.shape[0]
                        t2 = time.perf_counter()
                        timing['stage_copy_s'] += t2 - t1
                        with torch.cuda.stream(self.copy_stream):
                            dev = pin.to(self.device, non_blocking=True)
                            ready = torch.cuda.Event()
                            ready.record(self.copy_stream)
                        if n <= self.cap:
                            staged[k] = ready
                            k ^= 1
                        else:
                            ready.synchronize()
                        item['dev'], item['ready'] = dev, ready
                    else:
                        dev = torch.cat(pieces[0] + pieces[1])
                    free.put(sid)                           # the slab is free as soon as its contents sit in the staging buffer
                    views = [dev[off[c]:off[c + 1]] for c in range(2 * B)]
                    item['src_xyz'], item['tgt_xyz'] = views[:B], views[B:]
                    out.put(item)
                out.put(None)
            except BaseException as e:      # noqa: BLE001  (surface loader errors in the consumer)
                out.put(e)

        threading.Thread(target=dispatch, daemon=True).start()
        threading.Thread(target=upload, daemon=True).start()
        try:
            while True:
                t0 = time.perf_counter()
                b = out.get()
                timing['h2d_wait_s'] += time.perf_counter() - t0      # (time the CONSUMER stood waiting for a batch)
                if b is None:
                    return
                if isinstance(b, BaseException):
                    raise b
                if self.cuda:
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(b['ready'])
                    b['dev'].record_stream(cur)                 # allocated on the copy stream, consumed here
                yield b
        finally:
            sys.setswitchinterval(interval)                     # the process-wide switch interval is the caller's again

    def close(self):
        if self.pool is not None:
            self.pool.terminate(); self.pool.join()
            self.pool = None
        _POOL_SLABS.pop(self.pool_id, None)
        self._drop_source_file()
        self.slabs = []
        for m in self._maps:
            try:
                m.close()
            except BufferError:         # a numpy view still alive somewhere: the mapping goes with the process
                pass
        self._maps = []


class BatchLoader:
    """One pass of a LoaderPool created for it (and closed at the end): `for b in BatchLoader(pairs, indices, batch, device, workers)`."""

    def __init__(self, pairs, indices, batch, device, workers=4, depth=None, slab_points=None):
        self.pool = LoaderPool(pairs, device, workers=workers, max_batch=batch, depth=depth, slab_points=slab_points)
        self.indices, self.batch = indices, batch

    def __iter__(self):
        try:
            yield from self.pool.iterate(self.indices, self.batch)
        finally:
            self.pool.close()


# ------------------------------------------------------------------------------------------------------ result files
_POSE_FMT = ('\t'.join(['%.12f'] * 4) + '\n') * 4      # 4 rows, tab-separated, 12 decimals (generic_reg_model.py:279-281)


def write_est_log(log_path, benchmark, records, append=False):
    """generic_reg_model.py:260-281: per scene `<log_path>/<benchmark>/<scene>/est.log`, one block per pair:
    "{tgt_idx}\\t{src_idx}\\t-1" then the 4x4 pose, rows tab-separated with 12 decimals.
    A run writes each scene's file once, so the file is TRUNCATED unless append=True -- the reference opens it in append
    mode per pair (:276), which duplicates blocks (and corrupts the recall) when a run is repeated into the same log folder."""
    by_scene = {}
    for rec in records:
        scene = rec['src_path'].split(os.path.sep)[1]
        by_scene.setdefault(scene, []).append(rec)
    for scene, recs in by_scene.items():
        folder = os.path.join(log_path, benchmark, scene)
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, 'est.log'), 'a' if append else 'w') as fid:
            for rec in recs:
                src_idx = int(os.path.basename(rec['src_path']).split('_')[-1].replace('.pth', ''))
                tgt_idx = int(os.path.basename(rec['tgt_path']).split('_')[-1].replace('.pth', ''))
                pose = np.asarray(rec['pose'], dtype=np.float64)
                if pose.shape[0] == 3:
                    pose = np.concatenate([pose, [[0., 0., 0., 1.]]], axis=0)
                fid.write('{}\t{}\t{}\n'.format(tgt_idx, src_idx, -1) + _POSE_FMT % tuple(pose.ravel()))


def pose_errors(pred, gt):
    """Rotation error (deg) and translation error of (n, 3, 4) predictions against ground truth
    (utils/se3_torch.py se3_compare / generic_reg_model.py:198-210)."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    Rd = np.einsum('nij,nkj->nik', pred[:, :, :3], gt[:, :, :3])
    tr = np.clip((np.trace(Rd, axis1=1, axis2=2) - 1) / 2, -1, 1)
    return np.degrees(np.arccos(tr)), np.linalg.norm(pred[:, :, 3] - gt[:, :, 3], axis=1)


# ------------------------------------------------------------------------------------------------------ training input
def rank_batch_indices(n_items, batch_size, epochs, accumulate=1, rank=0, world=1, first_step=0):
    """THE BATCH SEQUENCE of accumulated / data-parallel training, as plain host arithmetic.  The unsharded run's batches are numbered
    j = 0, 1, ... across epochs (an epoch holds ceil(n_items / batch_size) of them).  Optimiser step s (from 1) with accumulate = k on
    W ranks consumes the k W micro-batches j = ((s - 1) k + m) W + r, micro-step m on rank r: rank r gets the j with j % W == r, up to
    the last COMPLETE group of k W batches -- a count every rank knows without communication.  first_step counts micro-batches: the
    j below it are left out.  -> rank r's j, ascending.  (k, W) and (k W, 1) therefore average the same micro-batches per step."""
    k, W = int(accumulate), int(world)
    if k < 1 or W < 1 or not 0 <= int(rank) < W:
        raise ValueError(f'accumulate >= 1, world >= 1 and 0 <= rank < world expected, got {accumulate}, {world}, {rank}')
    total = int(epochs) * -(-int(n_items) // int(batch_size))
    stop = total // (k * W) * (k * W)
    return [j for j in range(int(first_step), stop) if j % W == int(rank)]


def _epoch_batches(order, batch_size, epoch_first, wanted):
    """The part of one epoch's visiting order that makes up the batches `wanted` (a set of global batch indices), and those indices in
    order.  epoch_first: the index of the epoch's first batch.  Only the epoch's last batch can be short, so cutting the result into
    batch_size pieces again gives back exactly the wanted batches."""
    keep, js = [], []
    for b in range(-(-len(order) // batch_size)):
        if epoch_first + b in wanted:
            keep += order[b * batch_size:(b + 1) * batch_size]
            js.append(epoch_first + b)
    return keep, js


def train_batches(source, cfg, batch_size, seed, epochs=1, device=None, num_workers=4, loader_pool=None, first_step=0, accumulate=1,
                  rank=0, world=1):
    """Generator of augmented training batches over a 3DMatch-style pair source (`source[i]` -> {'src_xyz', 'tgt_xyz', 'pose', 'idx'}:
    ThreeDMatchPairs, SyntheticPairs): the loader pool, pinned staging and side-stream H2D copy run_test reads its pairs through, then
    augment.train_batch on the resident raw clouds -- overlap masks of the clean pair, the reference's augmentation chain -- with
    `step` counting up from 0 across epochs, so batch k of a run is a function of (source, seed, k) alone.  Every epoch visits every pair
    once in an order drawn from (seed, epoch); a last short batch is yielded as it is.  loader_pool: a LoaderPool over `source` made by the
    caller (e.g. before the GPU was initialised); else one of num_workers processes is made here and closed at the end (0: one loader
    thread).  Each batch goes straight into RegTR.training_step; 'ids' names its pairs.  first_step: start the (seed, step) sequence at
    that batch (a resumed run): batches 0 .. first_step - 1 are neither loaded nor built, batch first_step is the one an unbroken run
    yields there.  accumulate, rank, world: this rank's share of THE BATCH SEQUENCE (rank_batch_indices): only the batches j with
    j % world == rank, up to the last complete group of accumulate x world, are loaded and built -- each still from (seed, j), so batch j
    is the batch an unsharded run builds at j; first_step keeps counting micro-batches j.  The defaults yield every batch."""
    from .augment import train_batch
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    wanted = set(rank_batch_indices(len(source), batch_size, epochs, accumulate, rank, world, first_step))
    per_epoch = -(-len(source) // int(batch_size))
    pool = loader_pool
    if pool is None and num_workers > 0:
        pool = LoaderPool(source, device, workers=num_workers, max_batch=batch_size)
    try:
        for epoch in range(int(epochs)):
            order = np.random.default_rng([int(seed) & ((1 << 64) - 1), epoch]).permutation(len(source)).tolist()
            order, js = _epoch_batches(order, int(batch_size), epoch * per_epoch, wanted)
            if not order:
                continue
            loader = pool.iterate(order, batch_size) if pool is not None else Prefetcher(source, order, batch_size, device)
            for b, step in zip(loader, js):            # (the loader first: it is run to its end, as many batches as js has entries)
                gp = b['gt_pose'] if 'gt_pose' in b else [i_['pose'] for i_ in b['items']]
                if any(g_ is None for g_ in gp):
                    raise RuntimeError('train_batches: the pair source gives no ground-truth pose')
                pose = torch.from_numpy(np.stack([np.asarray(g_, dtype=np.float32)[:3] for g_ in gp])).to(device, non_blocking=True)
                out = train_batch(b['src_xyz'], b['tgt_xyz'], pose, cfg, seed, step)
                out['ids'] = b['ids'] if 'ids' in b else [i_['idx'] for i_ in b['items']]
                yield out
    finally:
        if pool is not None and loader_pool is None:
            pool.close()


def modelnet_train_batches(source, cfg, batch_size, seed, epochs=1, device=None, first_step=0, accumulate=1, rank=0, world=1):
    """Generator of ModelNet training batches over any indexable source of (n, 3) arrays (`source[i]`; further columns such as ModelNet40's
    normals are dropped, data_loaders/modelnet.py:176-177): the clouds of a batch go to the device in one pinned copy, then
    augment.modelnet_train_batch builds the cropped, moved, resampled, jittered and shuffled pairs with their masks and pose there.
    `step` counts up from 0 across epochs, so batch k of a run is a function of (source, seed, k) alone.  Every epoch visits every cloud
    once in an order drawn from (seed, epoch); a last short batch is yielded as it is.  Each batch goes straight into
    RegTR.training_step; 'ids' names its clouds.  (A 2048-point cloud is 24 KB: there is nothing for a loader pool to hide.  No HDF5
    reader here: hand in the arrays.)  first_step, accumulate, rank, world: as train_batches'."""
    from .augment import modelnet_train_batch
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    wanted = set(rank_batch_indices(len(source), batch_size, epochs, accumulate, rank, world, first_step))
    per_epoch = -(-len(source) // int(batch_size))
    for epoch in range(int(epochs)):
        order = np.random.default_rng([int(seed) & ((1 << 64) - 1), epoch]).permutation(len(source)).tolist()
        order, js = _epoch_batches(order, int(batch_size), epoch * per_epoch, wanted)
        for step, lo in zip(js, range(0, len(order), int(batch_size))):
            ids = order[lo:lo + int(batch_size)]
            clouds = [np.ascontiguousarray(np.asarray(source[i], dtype=np.float32)[:, :3]) for i in ids]
            lens = [len(c) for c in clouds]
            flat = torch.from_numpy(np.concatenate(clouds, axis=0))
            if device.type == 'cuda':
                flat = flat.pin_memory()
            out = modelnet_train_batch(list(torch.split(flat.to(device, non_blocking=True), lens)), cfg, seed, step)
            out['ids'] = ids
            yield out


# ------------------------------------------------------------------------------------------------------ the training loop
class CheckpointSaver:
    """The reference's CheckPointManager layout (cvhelpers/torch_helpers.py:98-193): `<dir>/model-<step>.pth`, one torch.save of
    {'state_dict', 'step', 'optimizer', 'scheduler'}, and `<dir>/checkpoints.txt` whose first line is `Best step: N` (the step of the
    highest score so far, the later one on a tie) followed by the kept files' names; the last max_to_keep checkpoints and the best one
    are kept.  load() takes a file or such a directory (the best step's file then), as the reference's --resume does."""

    def __init__(self, ckpt_dir, max_to_keep=3):
        self.dir, self.max_to_keep = ckpt_dir, int(max_to_keep)
        self.kept, self.best_score, self.best_step = [], None, None
        os.makedirs(ckpt_dir, exist_ok=True)

    def _path(self, step):
        return os.path.join(self.dir, f'model-{step}.pth')

    def save(self, model, step, score=0.0, **kwargs):
        state = {'state_dict': {k: v for k, v in model.state_dict().items() if not v.is_sparse}, 'step': step}
        for k, v in kwargs.items():
            state[k] = v.state_dict() if getattr(v, 'state_dict', None) is not None else v
        torch.save(state, self._path(step))
        self.kept.append(step)
        if self.best_score is None or score >= self.best_score:
            old = self.best_step
            self.best_score, self.best_step = score, step
            if old is not None and old not in self.kept and os.path.exists(self._path(old)):
                os.remove(self._path(old))
        while len(self.kept) > self.max_to_keep:
            gone = self.kept.pop(0)
            if gone != self.best_step:
                os.remove(self._path(gone))
        with open(os.path.join(self.dir, 'checkpoints.txt'), 'w') as f:
            f.write(f'Best step: {self.best_step}\n')
            f.write('\n'.join(os.path.basename(self._path(k)) for k in self.kept))
        return self._path(step)

    @staticmethod
    def load(path, model=None, map_location=None, **kwargs):
        """-> the checkpoint's step.  model: load_state_dict(strict=False), as the reference; kwargs (optimizer=, scheduler=): their
        load_state_dict with the entry of the same name, where the checkpoint has one."""
        if os.path.isdir(path):
            with open(os.path.join(path, 'checkpoints.txt')) as f:
                line = f.readline()
            if not line.startswith('Best'):
                raise RuntimeError(f'{path}/checkpoints.txt is not in the expected format (first line: Best step: N)')
            path = os.path.join(path, f'model-{int(line.split(":")[1])}.pth')
        state = torch.load(path, map_location=map_location, weights_only=False)
        if model is not None and 'state_dict' in state:
            model.load_state_dict(state['state_dict'], strict=False)
        for k, obj in kwargs.items():
            if k in state and getattr(obj, 'load_state_dict', None) is not None:
                obj.load_state_dict(state[k])
        return int(state.get('step', 0))

    @staticmethod
    def counters(path):
        """The 'nonfinite_guard' entry of a checkpoint written by train_loop(skip_nonfinite=True) -- {'skipped_steps',
        'skipped_micro_batches'} -- or None."""
        if os.path.isdir(path):
            with open(os.path.join(path, 'checkpoints.txt')) as f:
                path = os.path.join(path, f'model-{int(f.readline().split(":")[1])}.pth')
        return torch.load(path, map_location='cpu', weights_only=False).get('nonfinite_guard', None)

    @staticmethod
    def batching(path):
        """(accumulate, world) a checkpoint (a file, or a directory as load() takes it) was written with; (1, 1) for a checkpoint of the
        plain loop, which carries neither key."""
        if os.path.isdir(path):
            with open(os.path.join(path, 'checkpoints.txt')) as f:
                path = os.path.join(path, f'model-{int(f.readline().split(":")[1])}.pth')
        state = torch.load(path, map_location='cpu', weights_only=False)
        return int(state.get('accumulate', 1)), int(state.get('world', 1))


def _validate(model, val_batches):
    """validation_step over this rank's share of the validation batches (batch i on rank i % world), the per-batch outputs gathered to
    every rank in batch order by one all_gather_object (regtr_amd.distributed.gather_in_order; as host tensors, put back on their
    device), then validation_epoch_end: every rank computes the same score.  Without a process group: the plain loop over all batches."""
    from .distributed import gather_in_order, rank_world
    rank, world = rank_world()
    if world == 1 and not torch.distributed.is_initialized():
        return model.validation_epoch_end([model.validation_step(vb, i) for i, vb in enumerate(val_batches())])
    mine, dev = [], None
    for i, vb in enumerate(val_batches()):
        if i % world != rank:
            continue
        out = model.validation_step(vb, i)
        dev = next(iter(out[0].values())).device
        mine.append((i, tuple({k: v.cpu() for k, v in d.items()} for d in out)))
    outputs = gather_in_order(mine)
    if dev is None and outputs:              # (a rank without a batch of its own)
        dev = next(model.parameters()).device
    return model.validation_epoch_end([tuple({k: v.to(dev) for k, v in d.items()} for d in out) for out in outputs])


def train_loop(model, batches, steps, first_step=0, train_backbone=True, validate_every=0, val_batches=None, saver=None, logger=None,
               log_every=50, accumulate=1, skip_nonfinite=False, counters=None):
    """The reference's training loop (trainer.py:95-161) without tqdm and tensorboard: for each of `steps` batches of the iterable
    `batches` -- optimizer.zero_grad(), RegTR.training_step, backward, optimizer.step() (the gradient clip is inside it),
    scheduler.step() -- with model.optimizer / model.scheduler from RegTR.configure_optimizers (called here if the model has none yet).
    The global step starts at first_step (a resumed run: hand in batches that start there too).  Every loss key's running sum stays on
    the device, and so does the smoothed total (0.99 / 0.01, a non-finite total left out, as the reference); ONE host read per
    log_every steps prints it.  validate_every > 0 with val_batches (a callable returning an iterable of batches): every
    validate_every-th global step runs validation_step over them, validation_epoch_end, and saver.save(model, step, score,
    optimizer=, scheduler=) (a CheckpointSaver).  -> {'step', 'loss_smooth' (device scalar), 'loss_avg' {key: device scalar},
    'scores' [(step, score)], 'validation' the last validation_epoch_end outputs}.
    accumulate = k > 1, or an initialised process group (W ranks; `batches` is then this rank's share, train_batches(..., accumulate=,
    rank=, world=)): THE BUCKET PATH.  An optimiser step is k x (training_step, backward, GradBucket.add(1 / (k W), the stacked
    losses), gradients back to None), ONE all-reduce of the flat bucket, GradBucket.attach(), optimizer.step(), scheduler.step(); `steps`
    and the global step count optimiser steps, and the logged and averaged losses are the bucket tail's: the mean over the step's micro-
    batches and ranks.  Rank 0's parameters are broadcast once at the start; validation is sharded over the ranks (_validate) and rank 0
    alone logs and saves -- checkpoints then carry 'accumulate' and 'world'.  With accumulate == 1 and no process group the loop is
    the plain one: no bucket, the same launches, the same four checkpoint keys.
    skip_nonfinite=True (off: everything above, launch for launch): the optimiser must be a FusedAdamW(skip_nonfinite=True) (the config
    key `skip_nonfinite` makes configure_optimizers build one) and the bucket path uses GradBucket(skip_nonfinite=True): a step whose
    gradient is not finite is left out on the device, a micro-batch whose gradient is not finite is left out of the bucket, and the host
    is never asked.  The scheduler, the global step and the batch sequence advance on a skipped step (GradScaler's semantics).  Loss
    statistics then are finite-only: per key a sum and a count on the device -- on the bucket path the tail carries
    [where(isfinite(l), l, 0) ..., isfinite(l) ...] and the means are ratios taken after the all-reduce; on the plain path a skipped
    step's losses are left out as an excluded micro-batch's are -- so loss_avg[k] is the mean over the finite values and NaN only when
    there are none.  The result gains 'skipped_steps' and 'skipped_micro_batches' (device scalars, cumulative from `counters`, a
    {'skipped_steps', 'skipped_micro_batches'} dict of a resumed run's checkpoint); the log line prints both from its one host read;
    checkpoints carry them as 'nonfinite_guard'."""
    if getattr(model, 'optimizer', None) is None:
        model.configure_optimizers(train_backbone=train_backbone)
    opt, sched = model.optimizer, model.scheduler
    step = int(first_step)
    sums, smooth, n_done, scores, last_val = {}, None, 0, [], None
    guarded = bool(skip_nonfinite)
    if guarded and not getattr(opt, 'skip_nonfinite', False):
        raise RuntimeError('train_loop(skip_nonfinite=True) needs an optimiser built with skip_nonfinite=True (FusedAdamW; the config key '
                           '`skip_nonfinite` makes RegTR.configure_optimizers build one)')
    fin_sum = fin_cnt = None              # guarded: per key, the finite-only sum and count (device vectors in `keys` order)
    base = {k_: float((counters or {}).get(k_, 0)) for k_ in ('skipped_steps', 'skipped_micro_batches')}
    opt_skipped0 = None                   # the optimiser's cumulative count when this loop took its first step

    def skipped():
        """(skipped_steps, skipped_micro_batches) as float32 device scalars, cumulative over the run and its resumed ancestors."""
        s_ = opt.skipped_steps.to(torch.float32) - opt_skipped0 + base['skipped_steps']
        if bucket is not None:
            return s_, bucket.skipped_micro_batches + base['skipped_micro_batches']
        return s_, s_ - base['skipped_steps'] + base['skipped_micro_batches']
    it = iter(batches)
    from .distributed import broadcast_parameters, rank_world
    n_acc = int(accumulate)
    if n_acc < 1:
        raise ValueError(f'train_loop: accumulate must be at least 1, got {accumulate}')
    rank, world = rank_world()
    grouped = torch.distributed.is_available() and torch.distributed.is_initialized()
    bucketed = n_acc > 1 or grouped
    bucket, keys = None, None
    extra_ckpt = {'accumulate': n_acc, 'world': world} if n_acc * world > 1 else {}
    if grouped:
        broadcast_parameters(model)
    if rank != 0:
        logger, saver = None, None
    while n_done < int(steps):
        if bucketed:
            for _ in range(n_acc):
                try:
                    batch = next(it)
                except StopIteration:        # (the generators end on a complete group; an iterable that ends inside one ends the run,
                    batch = None             #  and that group's micro-batches are dropped)
                    break
                opt.zero_grad()
                _, losses = model.training_step(batch, step + 1, train_backbone=train_backbone)
                losses['total'].backward()
                if bucket is None:
                    from .grad_bucket import GradBucket
                    keys = list(losses)
                    bucket = GradBucket(list(model.named_parameters()), n_extra=len(keys) * (2 if guarded else 1), skip_nonfinite=guarded)
                stacked = torch.stack([losses[k_].detach() for k_ in keys])
                if guarded:
                    fin = torch.isfinite(stacked)
                    stacked = torch.cat([torch.where(fin, stacked, torch.zeros_like(stacked)), fin.to(stacked.dtype)])
                bucket.add(1.0 / (n_acc * world), stacked)
            opt.zero_grad()
            if batch is None:
                if bucket is not None:
                    bucket.reset()           # (the incomplete group's partial sums are not a step)
                break
            step += 1
            bucket.all_reduce()
            if guarded:
                bucket.attach(n_acc * world, opt)
                if opt_skipped0 is None:
                    opt_skipped0 = opt.skipped_steps.to(torch.float32).clone() if opt.skipped_steps is not None else 0.0
            else:
                bucket.attach()
            opt.step()
            sched.step()
            if guarded:
                tail = bucket.extra().clone()
                step_sum, step_cnt = tail[:len(keys)], tail[len(keys):]       # (both carry the 1 / (k W) of add(): the ratio does not)
                losses = dict(zip(keys, (step_sum / step_cnt).unbind(0)))     # (no finite value: 0 / 0 = NaN)
            else:
                losses = dict(zip(keys, bucket.extra().clone().unbind(0)))
        else:
            try:
                batch = next(it)
            except StopIteration:
                break
            step += 1
            opt.zero_grad()
            _, losses = model.training_step(batch, step, train_backbone=train_backbone)
            losses['total'].backward()
            if guarded and opt_skipped0 is None:
                opt_skipped0 = opt.skipped_steps.to(torch.float32).clone() if opt.skipped_steps is not None else 0.0
            opt.step()
            sched.step()
            if guarded:
                if keys is None:
                    keys = list(losses)
                stacked = torch.stack([losses[k_].detach() for k_ in keys])
                fin = torch.isfinite(stacked) & (opt.last_step_applied != 0)  # (a skipped step's losses are left out, as the bucket does)
                step_sum, step_cnt = torch.where(fin, stacked, torch.zeros_like(stacked)), fin.to(stacked.dtype)
        n_done += 1
        with torch.no_grad():
            if guarded:
                fin_sum = step_sum.clone() if fin_sum is None else fin_sum + step_sum
                fin_cnt = step_cnt.clone() if fin_cnt is None else fin_cnt + step_cnt
            for k, v in ({} if guarded else losses).items():
                v = v.detach()
                sums[k] = v.clone() if k not in sums else sums[k] + v
            total = losses['total'].detach()
            smooth = total.clone() if smooth is None else torch.where(torch.isfinite(total), 0.99 * smooth + 0.01 * total, smooth)
        if logger is not None and (n_done == 1 or step % int(log_every) == 0):
            if guarded:
                sm_, ss_, sb_ = torch.stack([smooth.to(torch.float32), *skipped()]).tolist()      # the one host read
                logger.info(f'step {step}: smoothed total loss {sm_:.4g}, lr {opt.param_groups[0]["lr"]:.3g}, skipped steps {int(ss_)}, '
                            f'skipped micro-batches {int(sb_)}')
            else:
                logger.info(f'step {step}: smoothed total loss {smooth.item():.4g}, lr {opt.param_groups[0]["lr"]:.3g}')      # the one host read
        if validate_every > 0 and val_batches is not None and step % int(validate_every) == 0:
            score, last_val = _validate(model, val_batches)
            scores.append((step, score))
            if logger is not None:
                logger.info(f'validation at step {step}: score {score:.4f}, total loss {float(last_val["losses"]["total"]):.4g}')
            if saver is not None:
                if guarded:
                    extra_ckpt['nonfinite_guard'] = dict(zip(('skipped_steps', 'skipped_micro_batches'), (int(x) for x in skipped())))
                path = saver.save(model, step, score, optimizer=opt, scheduler=sched, **extra_ckpt)
                if logger is not None:
                    logger.info(f'Saved checkpoint: {path} (best step {saver.best_step})')
    if guarded:
        out = {'step': step, 'loss_smooth': smooth, 'scores': scores, 'validation': last_val,
               'loss_avg': dict(zip(keys, (fin_sum / fin_cnt).unbind(0))) if fin_sum is not None else {}}
        if opt_skipped0 is None:          # (no step was taken)
            dev = next(model.parameters()).device
            out['skipped_steps'] = torch.tensor(base['skipped_steps'], device=dev)
            out['skipped_micro_batches'] = torch.tensor(base['skipped_micro_batches'], device=dev)
        else:
            out['skipped_steps'], out['skipped_micro_batches'] = skipped()
        return out
    return {'step': step, 'loss_smooth': smooth, 'loss_avg': {k: v / max(n_done, 1) for k, v in sums.items()}, 'scores': scores,
            'validation': last_val}


# ------------------------------------------------------------------------------------------------------ the test loop
def run_test(model, pairs, batch, device, logger=None, max_pairs=None, num_workers=0, loader_pool=None, losses=False, refine=None):
    """Runs every pair of `pairs` (this rank's shard) through the model, B at a time.  loader_pool: a LoaderPool over `pairs` (loader
    processes forked by the caller, e.g. before the GPU was initialised); else num_workers > 0: a pool forked here for this pass;
    0: one loader thread (Prefetcher).
    model: one RegTR module, or a LIST of replicas with the same weights (regtr_amd.workload.replicate): R host threads then take batches off the
    one loader in turn and run them on R HIP streams -- forwards in flight fill each other's host waits and heads (round 6; bench.py measures
    +6 % for three 64-pair forwards in flight); the poses come back in pair-id order either way, bit-identical to the one-replica run.
    losses: also RegTR.compute_loss(per_pair=True) of every pair (3DMatch-style pair sources: GT pose per pair, level-0 masks from
    overlap.compute_overlap_masks at cfg.overlap_radius); the means over all pairs of all ranks (one extra all-reduce) are returned in
    timing['losses'].  Without it the launches and outputs are those of a plain run.
    refine: None, or {'max_dist', 'iters'[, 'method', 'normal_radius']}: every batch's last-layer pose is polished on the batch's raw
    clouds by RegTR.refine_pose (ICP, regtr_amd/refine.py; point to point unless method says 'point_to_plane') on the stream of its forward, one model or replicas alike; the REFINED poses are returned
    and timing['refine'] holds the means over all pairs of all ranks of fitness and inlier_rmse before and after.  None: no launch and
    no output of a plain run changes.
    Returns, on every rank, (poses (n_total, 3, 4) float32 numpy ordered by pair id, pair ids, timing dict)."""
    import contextlib
    import itertools
    import threading
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    n = len(pairs) if max_pairs is None else min(len(pairs), max_pairs)
    mine = shard_pairs(n, rank, world)
    models = list(model) if isinstance(model, (list, tuple)) else [model]
    for m in models:
        m.eval()
    t0 = time.perf_counter()
    if loader_pool is not None:
        loader = loader_pool.iterate(mine, batch)
    else:
        loader = BatchLoader(pairs, mine, batch, device, workers=num_workers) if num_workers > 0 else Prefetcher(pairs, mine, batch, device)
    cuda = device.type == 'cuda'
    R = len(models)
    streams = [torch.cuda.Stream(device) for _ in range(R)] if (cuda and R > 1) else [None] * R
    it, turn, counter = iter(loader), threading.Lock(), itertools.count()
    done, errs, fwd_ms, loss_done, refine_done = [], [], [], [], []
    if refine is not None and not {'max_dist', 'iters'} <= set(refine) <= {'max_dist', 'iters', 'method', 'normal_radius'}:
        raise ValueError(f"run_test(refine=...): a dict with 'max_dist' and 'iters' (and at most 'method', 'normal_radius') expected, got {sorted(refine)}")
    if losses:
        if any(m.cfg.get('dataset', '3dmatch') != '3dmatch' for m in models):
            raise NotImplementedError('run_test(losses=True): ModelNet losses are not implemented (3DMatch-style pair sources only)')
        from .overlap import compute_overlap_masks

    def work(r):
        try:
            ctx = (torch.cuda.stream(streams[r]) if streams[r] is not None else contextlib.nullcontext())
            dctx = torch.cuda.device(device) if cuda else contextlib.nullcontext()
            with dctx, ctx, torch.no_grad():
                while not errs:
                    with turn:                                     # one loader, R consumers: batches are handed out in order
                        try:
                            b = next(it)
                        except StopIteration:
                            return
                        k = next(counter)
                    t_f = time.perf_counter()
                    fb = {'src_xyz': b['src_xyz'], 'tgt_xyz': b['tgt_xyz']}
                    out = models[r](fb)
                    fwd_ms.append(round((time.perf_counter() - t_f) * 1e3, 1))
                    if losses:
                        gp = b['gt_pose'] if 'gt_pose' in b else [i_['pose'] for i_ in b['items']]
                        if any(g_ is None for g_ in gp):
                            raise RuntimeError('run_test(losses=True): the pair source gives no ground-truth pose')
                        pose = torch.from_numpy(np.stack([np.asarray(g_, dtype=np.float32)[:3] for g_ in gp])).to(device, non_blocking=True)
                        sm, tm = compute_overlap_masks(b['src_xyz'], b['tgt_xyz'], pose, models[r].cfg.overlap_radius)
                        lo = models[r].compute_loss(out, {'kpconv_meta': fb['kpconv_meta'], 'pose': pose, 'src_overlap': sm,
                                                          'tgt_overlap': tm}, per_pair=True)
                        loss_done.append((k, list(lo), torch.stack([v_.to(torch.float64) for v_ in lo.values()])))     # (keys, B)
                    if refine is not None:
                        from . import refine as refine_
                        before = refine_.evaluate_registration(b['src_xyz'], b['tgt_xyz'], out['pose'][-1], refine['max_dist'])
                        res = models[r].refine_pose(fb, out['pose'][-1], max_dist=refine['max_dist'], iters=refine['iters'],
                                                    **{k_: refine[k_] for k_ in ('method', 'normal_radius') if k_ in refine})
                        refine_done.append((k, torch.stack([before[0], before[1], res.fitness, res.inlier_rmse])))      # (4, B) float64
                        out = {'pose': res.pose[None]}
                    done.append((k, out['pose'][-1], b['ids'] if 'ids' in b else [i_['idx'] for i_ in b['items']]))      # (B, 3, 4), stays on the device
        except BaseException as e:      # noqa: BLE001  (re-raised on the caller)
            errs.append(e)
    if R == 1:
        work(0)
    else:
        cur = torch.cuda.current_stream(device) if cuda else None
        th = [threading.Thread(target=work, args=(r,)) for r in range(R)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for s_ in streams:
            if s_ is not None:
                cur.wait_stream(s_)
        for _, p_, _ in done:
            if cuda:
                p_.record_stream(cur)
    if errs:
        raise errs[0]
    done.sort(key=lambda d: d[0])
    poses = [d[1] for d in done]
    ids = [i for d in done for i in d[2]]
    pose_t = torch.cat(poses).reshape(-1, 12) if poses else torch.zeros((0, 12), dtype=torch.float32, device=device)
    id_t = torch.tensor(ids, dtype=torch.int32, device=device)
    all_poses, all_ids = gather_poses(pose_t, id_t, n)
    loss_means = None
    if losses:
        loss_done.sort(key=lambda d: d[0])
        keys = loss_done[0][1] if loss_done else models[0].loss_keys()
        per = torch.cat([d[2] for d in loss_done], dim=1) if loss_done else torch.zeros((len(keys), 0), dtype=torch.float64, device=device)
        red = torch.cat([per.sum(dim=1), torch.tensor([float(per.shape[1])], dtype=torch.float64).to(device, non_blocking=True)])
        if world > 1:
            dist.all_reduce(red)                   # per-term sums and the pair count of every rank
        red = red.cpu().numpy()
        loss_means = {k_: float(red[j] / red[-1]) if red[-1] > 0 else float('nan') for j, k_ in enumerate(keys)}
    refine_means = None
    if refine is not None:
        refine_done.sort(key=lambda d: d[0])
        per = torch.cat([d[1] for d in refine_done], dim=1) if refine_done else torch.zeros((4, 0), dtype=torch.float64, device=device)
        red = torch.cat([per.sum(dim=1), torch.tensor([float(per.shape[1])], dtype=torch.float64).to(device, non_blocking=True)])
        if world > 1:
            dist.all_reduce(red)
        red = red.cpu().numpy()
        refine_means = {k_: float(red[j] / red[-1]) if red[-1] > 0 else float('nan')
                        for j, k_ in enumerate(('fitness_before', 'inlier_rmse_before', 'fitness_after', 'inlier_rmse_after'))}
    if device.type == 'cuda':
        torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - t0
    if logger and rank == 0:
        logger.info(f'{n} pairs on {world} GPU(s) in {elapsed:.2f} s = {n / elapsed:.1f} pairs/s (incl. loading)')
    poses_np = all_poses.reshape(-1, 3, 4).cpu().numpy()
    if not np.isfinite(poses_np).all():
        bad = np.unique(np.nonzero(~np.isfinite(poses_np))[0])
        raise RuntimeError(f'{len(bad)} of {len(poses_np)} predicted poses are not finite (first pair ids: {all_ids.cpu().numpy()[bad[:5]].tolist()}).  '
                           "(An f16 pair operand beyond 65504 is not the cause unless cfg.f16_range_check was switched off: RegTR.forward detects that "
                           "and re-runs the forward in fp32x3 arithmetic; compute_dtype: 'fp32x3' avoids the format altogether.)  Check the inputs "
                           'and the checkpoint for non-finite values.')
    timing = {'elapsed_s': elapsed, 'pairs': n, 'world': world, 'loader': getattr(loader_pool, 'last_timing', None), 'forward_ms': fwd_ms}
    if losses:
        timing['losses'] = loss_means
    if refine is not None:
        timing['refine'] = refine_means
    return poses_np, all_ids.cpu().numpy(), timing


# ------------------------------------------------------------------------------------------------------ the test loop on a cloud bank
def plan_windows(pair_keys, batch, max_bank_clouds):
    """The schedule of run_test_shared, pure Python: walks `pair_keys` -- a list of (src_key, tgt_key), any hashable keys -- in its given
    order, `batch` pairs per window, over a bank of at most max_bank_clouds clouds, and yields one dict per window:
        'first', 'count'   the window's pairs: pair_keys[first : first + count]
        'evict'            keys dropped from the bank before this window: the least recently used ones (by the last window that read
                           them; the older bank position first among equals), never one this window reads, and only as many as the bank
                           would otherwise exceed max_bank_clouds by
        'keep'             the surviving clouds' indices in the bank as it stood, ascending (CloudBank.select's argument); None when
                           nothing is evicted
        'encode'           keys to encode, in order of first appearance: the window's fragments that are not in the bank; they are
                           appended behind the surviving clouds
        'src', 'tgt'       per pair the bank index, in that new bank, of its source and its target
    ValueError when one window reads more distinct fragments than max_bank_clouds, naming the number it needs."""
    if batch < 1:
        raise ValueError(f'plan_windows: batch must be positive, got {batch}')
    bank, last_use = [], {}
    for w, first in enumerate(range(0, len(pair_keys), batch)):
        win = pair_keys[first:first + batch]
        need = list(dict.fromkeys(k for pair in win for k in pair))
        if len(need) > max_bank_clouds:
            raise ValueError(f'plan_windows: pairs {first} .. {first + len(win) - 1} read {len(need)} distinct fragments; max_bank_clouds must '
                             f'be at least {len(need)} (got {max_bank_clouds})')
        here = set(bank)
        encode = [k for k in need if k not in here]
        over = len(bank) + len(encode) - max_bank_clouds
        evict, keep = [], None
        if over > 0:
            wanted = set(need)
            cand = sorted((i for i, k in enumerate(bank) if k not in wanted), key=lambda i: (last_use[bank[i]], i))
            gone = set(cand[:over])
            evict = [bank[i] for i in cand[:over]]
            keep = [i for i in range(len(bank)) if i not in gone]
            bank = [bank[i] for i in keep]
            for k in evict:
                del last_use[k]
        bank = bank + encode
        at = {k: i for i, k in enumerate(bank)}
        for k in need:
            last_use[k] = w
        yield {'first': first, 'count': len(win), 'evict': evict, 'keep': keep, 'encode': encode,
               'src': [at[s] for s, _ in win], 'tgt': [at[t] for _, t in win]}


def run_test_shared(model, pairs, batch, device, logger=None, max_pairs=None, max_bank_clouds=1024, losses=False, refine=None):
    """run_test over a pair source that names its fragments (pairs.fragment_keys(i) -> (src_key, tgt_key), pairs.load_fragment(key) ->
    (n, 3) float32: ThreeDMatchPairs, SyntheticScenePairs), with every fragment's backbone run ONCE for as long as it stays in a bank of
    at most max_bank_clouds clouds: per window of `batch` pairs (plan_windows) the missing fragments are loaded and encoded in one
    RegTR.encode_clouds, joined to the bank (CloudBank.cat; on eviction CloudBank.select first) and the window's pairs registered in one
    RegTR.register.  A loader thread reads the next windows' missing fragments and copies them up on a side stream while the current
    window runs (as Prefetcher does for pairs; the LoaderPool processes are not used).  Under a process group every rank takes pairs i %
    world as run_test does and encodes the fragments of its own shard.  Returns what run_test returns, through gather_poses; timing
    additionally carries clouds_encoded, distinct_fragments and pair_slots (= 2 x pairs) of this rank.
    Refused: a list of replicas, losses=True, refine (ICP reads the raw clouds, which a bank need not hold)."""
    import torch.distributed as dist
    if refine is not None:
        raise NotImplementedError('run_test_shared: refine is not implemented on the shared path: ICP reads the raw clouds of a pair, and a '
                                  'cloud bank need not hold them (use run_test)')
    if isinstance(model, (list, tuple)):
        raise NotImplementedError('run_test_shared: replicas are not implemented on the shared path (one model, one stream)')
    if losses:
        raise NotImplementedError('run_test_shared: losses=True is not implemented on the shared path (use run_test)')
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('run_test_shared runs on an MI355X (HIP) device only; there is no CPU path')
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    n = len(pairs) if max_pairs is None else min(len(pairs), max_pairs)
    mine = shard_pairs(n, rank, world)
    model.eval()
    t0 = time.perf_counter()
    keys = [tuple(pairs.fragment_keys(i)) for i in mine]
    plan = list(plan_windows(keys, batch, max_bank_clouds))          # (a capacity below one window's need raises here, before any work)
    q = queue.Queue(maxsize=2)
    copy_stream = torch.cuda.Stream(device=device, priority=-1)
    stop = threading.Event()

    def load():
        try:
            for w in plan:
                if stop.is_set():
                    return
                host = [np.ascontiguousarray(pairs.load_fragment(k), dtype=np.float32) for k in w['encode']]
                item = {}
                with torch.cuda.stream(copy_stream):
                    item['clouds'] = [torch.from_numpy(a).pin_memory().to(device, non_blocking=True) for a in host]
                    item['ready'] = torch.cuda.Event()
                    item['ready'].record(copy_stream)
                q.put(item)
        except BaseException as e:      # noqa: BLE001  (surfaced in the consumer)
            q.put(e)
    th = threading.Thread(target=load, daemon=True)
    th.start()
    bank, done, win_ms = None, [], []
    try:
        with torch.cuda.device(device), torch.no_grad():
            for w in plan:
                item = q.get()
                if isinstance(item, BaseException):
                    raise item
                t_w = time.perf_counter()
                cur = torch.cuda.current_stream(device)
                cur.wait_event(item['ready'])
                for t in item['clouds']:                     # allocated on the copy stream
                    t.record_stream(cur)
                if w['keep'] is not None:
                    bank = bank.select(w['keep'])
                if item['clouds']:
                    new = model.encode_clouds(item['clouds'])
                    bank = new if bank is None else type(new).cat([bank, new])
                out = model.register(bank, w['src'], w['tgt'])
                done.append(out['pose'][-1])                 # (count, 3, 4), stays on the device
                win_ms.append(round((time.perf_counter() - t_w) * 1e3, 1))
    finally:
        stop.set()
        while th.is_alive():                                 # (a loader blocked on a full queue after an error here)
            try:
                q.get_nowait()
            except queue.Empty:
                pass
            th.join(timeout=0.05)
    pose_t = torch.cat(done).reshape(-1, 12) if done else torch.zeros((0, 12), dtype=torch.float32, device=device)
    id_t = torch.tensor(mine, dtype=torch.int32, device=device)
    all_poses, all_ids = gather_poses(pose_t, id_t, n)
    torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - t0
    encoded = sum(len(w['encode']) for w in plan)
    distinct = len({k for pair in keys for k in pair})
    if logger and rank == 0:
        logger.info(f'{n} pairs on {world} GPU(s) in {elapsed:.2f} s = {n / elapsed:.1f} pairs/s (incl. loading); rank 0 encoded {encoded} clouds '
                    f'for {2 * len(mine)} pair slots ({distinct} distinct fragments)')
    poses_np = all_poses.reshape(-1, 3, 4).cpu().numpy()
    if not np.isfinite(poses_np).all():
        bad = np.unique(np.nonzero(~np.isfinite(poses_np))[0])
        raise RuntimeError(f'{len(bad)} of {len(poses_np)} predicted poses are not finite (first pair ids: {all_ids.cpu().numpy()[bad[:5]].tolist()}); '
                           'check the inputs and the checkpoint for non-finite values')
    timing = {'elapsed_s': elapsed, 'pairs': n, 'world': world, 'loader': None, 'forward_ms': win_ms, 'clouds_encoded': encoded,
              'distinct_fragments': distinct, 'pair_slots': 2 * len(mine)}
    return poses_np, all_ids.cpu().numpy(), timing
