"""Training batches from a device-resident set of labelled part clouds.

``PartCloudSet`` keeps a ragged set of clouds (points, part labels) in device memory and assembles the collated item of the
reference's ``_ShapeNetSegParts.__getitem__`` (python/difffacto/datasets/shapenet_seg.py:436-543, ``pc_norm`` in
dataset_utils.py:55-95) for a whole batch with one workgroup per shape (libdfx's batch_kernels.hip).
``PartCloudLoader`` iterates over such batches.  The random inputs of an item (the resampling ``choice``, the part-dropout draws
``drop_u`` and the augmentation draws ``aug_u``) are explicit tensors; without them they come from Philox keyed by
``(seed, sample_id)``, so an item does not depend on its row in the batch or on the batch size.

Not served: the Runner / config-registry wiring, the other dataset classes, ``global_unit`` and normal channels.
"""
import json
import os

import numpy as np
import torch

from . import _ffi

SCALE_MODES = {None: 0, "none": 0, "shape_unit": 1, "shape_half": 2, "shape_34": 3, "shape_bbox": 4, "shape_canonical": 5,
               "shape_canonical_bbox": 6}
SHAPE_SCALE_MODES = (None, "none", "shape_unit", "shape_half", "shape_34", "shape_bbox")
MAX_CLASSES = 8
MIN_POINTS, MAX_POINTS = 10, 8192

# synset per class and the per-class part-label table of the ShapeNet part benchmark (shapenet_seg.py:19-39, :104-175): the label
# offset of a class is the first entry of its row, the number of parts the row's length
SHAPENET_SYNSETS = {"Airplane": "02691156", "Bag": "02773838", "Cap": "02954340", "Car": "02958343", "Chair": "03001627",
                    "Earphone": "03261776", "Guitar": "03467517", "Knife": "03624134", "Lamp": "03636649", "Laptop": "03642806",
                    "Motorbike": "03790512", "Mug": "03797390", "Pistol": "03948459", "Rocket": "04099429", "Skateboard": "04225987",
                    "Table": "04379243"}
SHAPENET_PART_LABELS = {"Earphone": [16, 17, 18], "Motorbike": [30, 31, 32, 33, 34, 35], "Rocket": [41, 42, 43], "Car": [8, 9, 10, 11],
                        "Laptop": [28, 29], "Cap": [6, 7], "Skateboard": [44, 45, 46], "Mug": [36, 37], "Guitar": [19, 20, 21],
                        "Bag": [4, 5], "Lamp": [24, 25, 26, 27], "Table": [47, 48, 49], "Airplane": [0, 1, 2, 3], "Pistol": [38, 39, 40],
                        "Chair": [12, 13, 14, 15], "Knife": [22, 23]}
_SPLIT_FILES = {"train": ("train",), "val": ("val",), "test": ("test",), "trainval": ("train", "val"), "all": ("train", "val", "test")}


_NUMPY_DTYPES = {torch.int64: np.int64, torch.int32: np.int32, torch.float32: np.float32}


def _upload(host, device):
    """A host array on ``device`` without draining the stream: a pinned staging copy and a non-blocking transfer.  (A blocking
    ``.to()`` from pageable memory makes the host wait for everything queued on the stream before it: inside a training loop that
    is the whole previous step.)  The caching host allocator keeps the staging block alive until the copy has run."""
    src = torch.from_numpy(np.ascontiguousarray(host))
    if torch.device(device).type == "cpu":
        return src
    return src.pin_memory().to(device, non_blocking=True)


def scale_mode_code(name, part=False):
    if name == "global_unit":
        raise NotImplementedError("scale mode 'global_unit' (data-set statistics) is not implemented")
    allowed = SCALE_MODES if part else SHAPE_SCALE_MODES
    if name not in allowed:
        raise ValueError(f"unknown {'part_' if part else ''}scale_mode {name!r}: one of {[m for m in allowed if m]}")
    return SCALE_MODES[name]


class BatchCheck:
    """The deferred validity check of a batch: ``n_bad`` (int32 (2), device) counts sampled labels outside [0, n_class) and items
    with an unusable index / cloud / choice.  ``raise_if_bad()`` reads it (one host sync)."""

    def __init__(self, n_bad, n_class):
        self.n_bad, self.n_class = n_bad, n_class

    def raise_if_bad(self):
        labels, items = (int(v) for v in self.n_bad.tolist())
        if items:
            raise IndexError(f"PartCloudSet.batch: {items} item(s) with an index outside the set, an empty cloud or a choice outside their cloud")
        if labels:
            raise ValueError(f"PartCloudSet.batch: {labels} sampled label(s) outside [0,{self.n_class})")


class PartCloudSet:
    """A ragged set of S labelled clouds: ``points`` (P,3) float32, ``labels`` (P,) int32, ``offsets`` (S+1,) int64."""

    def __init__(self, points, labels, offsets, n_class, tokens=None, class_id=0, device="cuda"):
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        labels = np.ascontiguousarray(labels, np.int32).reshape(-1)
        offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        S = len(offsets) - 1
        if S < 1 or offsets[0] != 0 or offsets[-1] != len(points) or len(labels) != len(points):
            raise ValueError("PartCloudSet: offsets must run from 0 to the number of points over at least one cloud")
        if np.any(np.diff(offsets) <= 0):
            raise ValueError(f"PartCloudSet: cloud {int(np.argmax(np.diff(offsets) <= 0))} is empty")
        if not 1 <= int(n_class) <= MAX_CLASSES:
            raise ValueError(f"PartCloudSet: n_class = {n_class} outside [1,{MAX_CLASSES}]")
        self.n_class, self.class_id = int(n_class), int(class_id)
        self.tokens = [str(t) for t in tokens] if tokens is not None else [str(i) for i in range(S)]
        if len(self.tokens) != S:
            raise ValueError(f"PartCloudSet: {len(self.tokens)} tokens for {S} clouds")
        self.host = (points, labels, offsets)
        self.device = torch.device(device)
        self.points, self.labels, self.offsets = (torch.from_numpy(a).to(self.device) for a in self.host)
        self.noise = None

    def __len__(self):
        return len(self.host[2]) - 1

    # ---- constructors ----
    @classmethod
    def from_arrays(cls, clouds, n_class, tokens=None, device="cuda", class_id=0):
        """``clouds``: a sequence of (points (M,3), labels (M,)) pairs."""
        pts = [np.asarray(p, np.float32).reshape(-1, 3) for p, _ in clouds]
        seg = [np.asarray(s).reshape(-1).astype(np.int32) for _, s in clouds]
        for k, (p, s) in enumerate(zip(pts, seg)):
            if len(p) != len(s):
                raise ValueError(f"PartCloudSet.from_arrays: cloud {k} has {len(p)} points and {len(s)} labels")
        offsets = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
        return cls(np.concatenate(pts) if pts else np.zeros((0, 3), np.float32), np.concatenate(seg) if seg else np.zeros(0, np.int32),
                   offsets, n_class, tokens, class_id, device)

    @classmethod
    def from_shapenet_dir(cls, root, class_choice="Chair", split="train", device="cuda"):
        """The txt layout of the ShapeNet part benchmark (shapenet_seg.py:104-160, :445-452): ``root/<synset>/<token>.txt`` with rows
        ``x y z nx ny nz label`` and ``root/train_test_split/shuffled_{train,val,test}_file_list.json``; files in sorted order,
        labels minus the class's first part label.  Parsed on the host, once."""
        if class_choice not in SHAPENET_SYNSETS:
            raise ValueError(f"from_shapenet_dir: unknown class {class_choice!r}")
        if split not in _SPLIT_FILES:
            raise ValueError(f"from_shapenet_dir: unknown split {split!r}: one of {sorted(_SPLIT_FILES)}")
        ids = set()
        for part in _SPLIT_FILES[split]:
            with open(os.path.join(root, "train_test_split", f"shuffled_{part}_file_list.json")) as f:
                ids |= {str(d.split("/")[2]) for d in json.load(f)}
        folder = os.path.join(root, SHAPENET_SYNSETS[class_choice])
        names = [fn for fn in sorted(os.listdir(folder)) if fn[:-4] in ids]
        if not names:
            raise ValueError(f"from_shapenet_dir: no file of split {split!r} under {folder}")
        first = SHAPENET_PART_LABELS[class_choice][0]
        clouds, tokens = [], []
        for fn in names:
            data = np.loadtxt(os.path.join(folder, fn), ndmin=2).astype(np.float32)
            clouds.append((data[:, 0:3], data[:, -1].astype(np.int64) - first))
            tokens.append(os.path.splitext(fn)[0])
        return cls.from_arrays(clouds, len(SHAPENET_PART_LABELS[class_choice]), tokens, device, list(SHAPENET_SYNSETS).index(class_choice))

    def save(self, path):
        points, labels, offsets = self.host
        np.savez(path, points=points, labels=labels, offsets=offsets, n_class=np.int64(self.n_class), class_id=np.int64(self.class_id),
                 tokens=np.asarray(self.tokens, dtype=str))

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path) as z:
            return cls(z["points"], z["labels"], z["offsets"], int(z["n_class"]), [str(t) for t in z["tokens"]], int(z["class_id"]), device)

    def set_noise(self, noise):
        """A (S, D) tensor whose rows travel with the items as ``noise`` (stage 2's cache_noise); None: (B,1) float64 zeros."""
        if noise is not None:
            noise = torch.as_tensor(noise).to(self.device)
            if noise.dim() != 2 or noise.shape[0] != len(self):
                raise ValueError(f"set_noise: shape {tuple(noise.shape)}, expected ({len(self)}, D)")
        self.noise = noise

    # ---- batches ----
    def _index(self, index):
        """-> (int64 tensor on the device, host copy or None).  A host index is range-checked here; a device index in the kernel."""
        if isinstance(index, torch.Tensor) and index.device.type != "cpu":
            return index.to(device=self.device, dtype=torch.int64).contiguous().reshape(-1), None
        host = np.asarray(index.numpy() if isinstance(index, torch.Tensor) else index, dtype=np.int64).reshape(-1)
        if host.size == 0:
            raise ValueError("PartCloudSet.batch: empty index")
        if host.min() < 0 or host.max() >= len(self):
            raise IndexError(f"PartCloudSet.batch: index outside [0,{len(self)})")
        return _upload(host, self.device), host

    def _explicit(self, t, shape, dtype, name):
        if isinstance(t, torch.Tensor) and t.device.type != "cpu":
            t = t.to(device=self.device, dtype=dtype).contiguous()
        else:   # host data: no blocking copy
            t = _upload(np.asarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=_NUMPY_DTYPES[dtype]), self.device)
        if tuple(t.shape) != shape:
            raise ValueError(f"PartCloudSet.batch: {name} of shape {tuple(t.shape)}, expected {shape}")
        return t

    def draw(self, index, sample_id, seed, npoints):
        """(choice int32 (B,N), drop_u float32 (B,C), aug_u float32 (B,6)) of ``dfx_batch_draw`` for device tensors index / sample_id."""
        B, C = index.numel(), self.n_class
        choice = torch.empty(B, npoints, dtype=torch.int32, device=self.device)
        drop_u = torch.empty(B, C, dtype=torch.float32, device=self.device)
        aug_u = torch.empty(B, 6, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _ffi.check(_ffi.lib().dfx_batch_draw(_ffi.ptr(self.offsets), len(self), _ffi.ptr(index), _ffi.ptr(sample_id), B, npoints, C,
                                                 int(seed) & (2 ** 64 - 1), _ffi.ptr(choice), _ffi.ptr(drop_u), _ffi.ptr(aug_u),
                                                 _ffi.current_stream()), "dfx_batch_draw")
        return choice, drop_u, aug_u

    def batch(self, index, sample_id=None, seed=None, choice=None, drop_u=None, aug_u=None, npoints=2048, scale_mode="shape_unit",
              part_scale_mode="shape_canonical", clip=False, dropout_part=0.0, augment=False, augment_shift=False, augment_scale=False,
              check=True):
        """The reference's collated item for the clouds ``index`` (B,), as device tensors.  Explicit draws win over ``seed``; with
        neither, a fresh key comes from ``engine.resolve_seed``.  ``sample_id`` (B,) int64 defaults to ``index``.
        ``shift`` is (B,1,3); ``scale`` is (B,1,1), and (B,1,3) with an augmentation (the reference's ``rand_scale * scale``).
        ``check=True`` raises for labels outside [0, n_class) (one host sync); ``check=False`` puts nothing but launches and
        non-blocking copies of host arguments (lists, arrays, CPU tensors: through pinned memory) on the current stream and returns
        the deferred check under the key ``"check"`` (``BatchCheck.raise_if_bad``)."""
        N, C = int(npoints), self.n_class
        if not MIN_POINTS <= N <= MAX_POINTS:
            raise ValueError(f"PartCloudSet.batch: npoints = {N} outside [{MIN_POINTS},{MAX_POINTS}]")
        part_scale_mode = scale_mode if part_scale_mode is None else part_scale_mode
        sm, pm = scale_mode_code(scale_mode), scale_mode_code(part_scale_mode, part=True)
        if augment:
            augment_shift = augment_scale = True
        idx, idx_host = self._index(index)
        B = idx.numel()
        if choice is None or drop_u is None or aug_u is None:
            from . import engine
            sid = idx if sample_id is None else self._explicit(sample_id, (B,), torch.int64, "sample_id")
            drawn = self.draw(idx, sid, engine.resolve_seed(seed), N)
            choice, drop_u, aug_u = (d if e is None else e for d, e in zip(drawn, (choice, drop_u, aug_u)))
        choice = self._explicit(choice, (B, N), torch.int32, "choice")
        drop_u = self._explicit(drop_u, (B, C), torch.float32, "drop_u")
        aug_u = self._explicit(aug_u, (B, 6), torch.float32, "aug_u")
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        ref, inp = torch.empty(B, N, 3, **f32), torch.empty(B, N, 3, **f32)
        seg = torch.empty(B, N, dtype=torch.int64, device=dev)
        attn = torch.empty(B, N, C, dtype=torch.int64, device=dev)
        present, dp_present = torch.empty(B, C, **f32), torch.empty(B, C, **f32)
        part_shift, part_scale = torch.empty(B, 3, C, **f32), torch.empty(B, 3, C, **f32)
        shift, scale = torch.empty(B, 1, 3, **f32), torch.empty(B, 1, 3, **f32)
        n_bad = torch.empty(2, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = _ffi.lib().dfx_batch_build_f32(
                _ffi.ptr(self.points), _ffi.ptr(self.labels), _ffi.ptr(self.offsets), len(self), _ffi.ptr(idx), B, _ffi.ptr(choice),
                _ffi.ptr(drop_u), _ffi.ptr(aug_u), C, N, sm, pm, int(bool(clip)), float(dropout_part), int(bool(augment_shift)),
                int(bool(augment_scale)), _ffi.ptr(ref), _ffi.ptr(inp), _ffi.ptr(seg), _ffi.ptr(attn), _ffi.ptr(present),
                _ffi.ptr(dp_present), _ffi.ptr(part_shift), _ffi.ptr(part_scale), _ffi.ptr(shift), _ffi.ptr(scale), _ffi.ptr(n_bad),
                _ffi.current_stream())
        _ffi.check(rc, "dfx_batch_build_f32")
        checker = BatchCheck(n_bad, C)
        if check:
            checker.raise_if_bad()
        if not (augment_shift or augment_scale):
            scale = scale[:, :, :1]
        noise = torch.zeros(B, 1, dtype=torch.float64, device=dev) if self.noise is None else self.noise.index_select(0, idx)
        tokens = [self.tokens[i] for i in idx_host] if idx_host is not None else None   # a device index: no host copy, no tokens
        out = {"present": present, "dp_present": dp_present, "part_scale": part_scale, "part_shift": part_shift, "input": inp, "ref": ref,
               "attn_map": attn, "ref_attn_map": attn, "ref_seg_mask": seg, "seg_mask": seg, "shift": shift, "scale": scale, "id": idx,
               "class": torch.full((B, 1), self.class_id, dtype=torch.int32, device=dev), "token": tokens, "noise": noise}
        if not check:
            out["check"] = checker
        return out


class PartCloudLoader:
    """Iterates over the batches of a ``PartCloudSet``: one pass per ``iter()``.  The order of epoch e is a permutation drawn from
    ``(seed, e)`` on the host and uploaded once per epoch (pinned, non-blocking); batches slice it on the device, and the item at
    position p of epoch e has ``sample_id = e * S + p`` (formed on the device), so a run is replayable from ``seed`` alone.
    ``check=False`` (the default here) keeps the host out of the stream: the batches' ``n_bad`` counters add up in one device
    tensor, which ``loader.raise_if_bad()`` reads (one host sync) and clears."""

    def __init__(self, dataset, batch_size, shuffle=True, drop_last=True, seed=None, check=False, **batch_options):
        for k in ("index", "sample_id", "choice", "drop_u", "aug_u"):
            if k in batch_options:
                raise TypeError(f"PartCloudLoader: {k} is the loader's to set")
        if batch_size < 1 or (drop_last and batch_size > len(dataset)):
            raise ValueError(f"PartCloudLoader: batch_size = {batch_size} with {len(dataset)} clouds")
        from . import engine
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), shuffle, drop_last
        self.seed = engine.resolve_seed(seed)
        self.check, self.options = check, batch_options
        self.epoch = 0
        self._bad = None

    def __len__(self):
        S = len(self.dataset)
        return S // self.batch_size if self.drop_last else -(-S // self.batch_size)

    def order(self, epoch):
        S = len(self.dataset)
        if not self.shuffle:
            return np.arange(S, dtype=np.int64)
        return np.random.Generator(np.random.PCG64([self.seed & (2 ** 64 - 1), int(epoch)])).permutation(S).astype(np.int64)

    def __iter__(self):
        ds, epoch, S = self.dataset, self.epoch, len(self.dataset)
        self.epoch += 1
        order = self.order(epoch)
        order_dev = _upload(order, ds.device)
        for k in range(len(self)):
            lo, hi = k * self.batch_size, min((k + 1) * self.batch_size, S)
            sample_id = torch.arange(epoch * S + lo, epoch * S + hi, dtype=torch.int64, device=ds.device)
            out = ds.batch(order_dev[lo:hi], sample_id=sample_id, seed=self.seed, check=self.check, **self.options)
            out["token"] = [ds.tokens[i] for i in order[lo:hi]]
            if not self.check:
                n_bad = out.pop("check").n_bad
                self._bad = n_bad if self._bad is None else self._bad.add_(n_bad)
            yield out

    def raise_if_bad(self):
        bad, self._bad = self._bad, None
        if bad is not None:
            BatchCheck(bad, self.dataset.n_class).raise_if_bad()
