"""On-disk dataset readers for the device input pipeline: the counterparts of the reference's
``load_cifar10`` / ``load_imagenet_subset`` (utils/data_utils.py:83-244).

The reference wraps torchvision's CIFAR10 / ImageFolder datasets in DataLoaders whose worker processes decode, crop
and resize every image with PIL.  Here the host only READS: CIFAR-10's binary distribution is one numpy read per file,
an image folder is decoded by a small thread pool into packed uint8 bytes (``data.RaggedBatch``: every photograph keeps
its own size), and crop / flip / resize / normalise run on the device (``data.DeviceTransform``).  Nothing downloads.
"""
from __future__ import annotations

import os
import queue
import threading
import weakref
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .data import DeviceLoader, RaggedBatch, get_transforms

CIFAR10_CLASSES = ["airplane", "automobile", "bird", "cat", "deer", "dog", "frog", "horse", "ship", "truck"]
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
MAX_WORKERS = 16           # decoding threads are never sized by the CPU count of the machine
_RECORD = 1 + 3 * 32 * 32  # CIFAR-10 binary record: label byte, then the R, G and B planes (row-major 32 x 32 each)


def _subset(n: int, subset_size: Optional[int], seed: int) -> Optional[np.ndarray]:
    """Indices of a seeded random subset (the reference: randperm(len)[:subset_size]); None = everything."""
    if subset_size is None:
        return None
    if subset_size < 0:
        raise ValueError("subset_size must not be negative")
    return np.random.RandomState(seed).permutation(n)[:subset_size]


class Cifar10Binary:
    """The binary CIFAR-10 distribution (data_batch_1..5.bin / test_batch.bin, optionally batches.meta.txt), found in
    ``data_dir`` or ``data_dir/cifar-10-batches-bin``.  x: uint8 [N,32,32,3] (HWC), y: int64 [N], both in host memory."""

    def __init__(self, data_dir: str, train: bool, subset_size: Optional[int] = None, seed: int = 0):
        if not os.path.isdir(data_dir):
            raise FileNotFoundError(f"CIFAR-10 directory not found: {data_dir}")
        names = [f"data_batch_{i}.bin" for i in range(1, 6)] if train else ["test_batch.bin"]
        root = None
        for cand in (data_dir, os.path.join(data_dir, "cifar-10-batches-bin")):
            if all(os.path.isfile(os.path.join(cand, n)) for n in names):
                root = cand
                break
        if root is None:
            py = [c for c in (os.path.join(data_dir, "cifar-10-batches-py"), data_dir)
                  if os.path.isfile(os.path.join(c, "data_batch_1")) or os.path.isfile(os.path.join(c, "test_batch"))]
            if py:
                raise FileNotFoundError(f"{py[0]} holds the pickled (python) CIFAR-10 distribution; the binary distribution "
                                        f"(cifar-10-batches-bin: {', '.join(names)}) is required -- pickles are not read")
            raise FileNotFoundError(f"CIFAR-10 binary files ({', '.join(names)}) not found in {data_dir} or "
                                    f"{os.path.join(data_dir, 'cifar-10-batches-bin')}")
        xs, ys = [], []
        for n in names:
            path = os.path.join(root, n)
            raw = np.fromfile(path, dtype=np.uint8)
            if raw.size == 0 or raw.size % _RECORD != 0:
                raise ValueError(f"{path}: {raw.size} bytes is not a multiple of the {_RECORD}-byte CIFAR-10 record")
            rec = raw.reshape(-1, _RECORD)
            if int(rec[:, 0].max()) > 9:
                r = int(np.argmax(rec[:, 0] > 9))
                raise ValueError(f"{path}: record {r} has label {int(rec[r, 0])} (CIFAR-10 labels are 0..9)")
            ys.append(rec[:, 0].astype(np.int64))
            xs.append(rec[:, 1:].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))        # planes -> HWC
        self.root, self.train = root, train
        self.x = np.ascontiguousarray(np.concatenate(xs))
        self.y = np.concatenate(ys)
        keep = _subset(len(self.y), subset_size, seed)
        if keep is not None:
            self.x, self.y = np.ascontiguousarray(self.x[keep]), self.y[keep]
        self.classes = list(CIFAR10_CLASSES)
        meta = os.path.join(root, "batches.meta.txt")
        if os.path.isfile(meta):
            with open(meta) as f:
                found = [ln.strip() for ln in f if ln.strip()]
            if len(found) == 10:
                self.classes = found

    def __len__(self) -> int:
        return len(self.y)


class ImageFolder:
    """torchvision's ImageFolder layout and ordering: classes are the sorted sub-directory names, samples the valid
    image files of each class directory walked in sorted order.  ``load(i)`` decodes sample i to a HWC uint8 RGB array."""

    def __init__(self, root: str, subset_size: Optional[int] = None, seed: int = 0):
        if not os.path.isdir(root):
            raise FileNotFoundError(f"image folder not found: {root}")
        self.root = root
        self.classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples: List[Tuple[str, int]] = []
        empty = []
        for c in self.classes:
            n0 = len(self.samples)
            for d, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for fn in sorted(files):
                    if fn.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(d, fn), self.class_to_idx[c]))
            if len(self.samples) == n0:
                empty.append(c)
        if empty:
            raise FileNotFoundError(f"Found no valid file for the classes {', '.join(empty)}. "
                                    f"Supported extensions are: {', '.join(IMG_EXTENSIONS)}")
        keep = _subset(len(self.samples), subset_size, seed)
        if keep is not None:
            self.samples = [self.samples[i] for i in keep]
        self.targets = np.array([t for _, t in self.samples], dtype=np.int64)

    def __len__(self) -> int:
        return len(self.samples)

    def load(self, i: int) -> np.ndarray:
        from PIL import Image
        with Image.open(self.samples[i][0]) as im:
            return np.asarray(im.convert("RGB"))


# ---------------------------------------------------------------- host batches ----
_END = object()


def _worker(jobs: "queue.Queue") -> None:
    while True:
        job = jobs.get()
        if job is None:
            return
        ds, i, out, k, done = job
        try:
            out[k] = ds.load(i)
        except BaseException as e:          # handed to the consumer, which re-raises it
            out[k] = e
        done.release()


def _produce(ds: ImageFolder, chunks: List[np.ndarray], out_q: "queue.Queue", stop: threading.Event, workers: int) -> None:
    """Decodes batch after batch with `workers` daemon threads and hands each to the bounded queue.  Holds no reference
    to the iterator, so an abandoned iterator is collected, sets `stop`, and everything here ends."""
    jobs: "queue.Queue" = queue.Queue()
    pool = [threading.Thread(target=_worker, args=(jobs,), daemon=True, name=f"favit-decode-{k}") for k in range(workers)]
    for t in pool:
        t.start()

    def hand_over(item) -> bool:
        while not stop.is_set():
            try:
                out_q.put(item, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    try:
        for idx in chunks:
            out: List[Any] = [None] * len(idx)
            done = threading.Semaphore(0)
            for k, i in enumerate(idx):
                jobs.put((ds, int(i), out, k, done))
            for _ in idx:
                while not done.acquire(timeout=0.05):
                    if stop.is_set():
                        return
            err = next((o for o in out if isinstance(o, BaseException)), None)
            if err is not None:
                hand_over(err)
                return
            if not hand_over((RaggedBatch.from_images(out), ds.targets[idx].copy())):
                return
        hand_over(_END)
    finally:
        while True:                          # drop what an abandoned epoch left queued, then release the workers
            try:
                jobs.get_nowait()
            except queue.Empty:
                break
        for _ in pool:
            jobs.put(None)


class _FolderEpoch:
    """Iterator over one epoch of an ImageFolder: one batch is decoded ahead of the consumer."""

    def __init__(self, ds: ImageFolder, chunks: List[np.ndarray], workers: int):
        self._q: "queue.Queue" = queue.Queue(maxsize=1)
        self._stop = threading.Event()
        self._done = False
        self._thread = threading.Thread(target=_produce, args=(ds, chunks, self._q, self._stop, workers), daemon=True,
                                        name="favit-batches")
        self._thread.start()
        weakref.finalize(self, self._stop.set)

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration
        item = self._q.get()
        if item is _END:
            self.close()
            raise StopIteration
        if isinstance(item, BaseException):
            self.close()
            raise item
        return item

    def close(self) -> None:
        self._done = True
        self._stop.set()


class _Batches:
    def __init__(self, dataset, batch_size: int, shuffle: bool, seed: int, drop_last: bool, num_workers: int):
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        if not isinstance(dataset, (Cifar10Binary, ImageFolder)):
            raise TypeError("batches() takes a Cifar10Binary or an ImageFolder")
        self.ds, self.bs, self.shuffle, self.seed, self.drop_last = dataset, int(batch_size), shuffle, int(seed), drop_last
        self.workers = max(1, min(int(num_workers), MAX_WORKERS))
        self.epoch = 0

    def __len__(self) -> int:
        n = len(self.ds)
        return n // self.bs if self.drop_last else (n + self.bs - 1) // self.bs

    # checkpoint state: the shuffle of epoch e is a function of (seed, e) alone
    def state_dict(self) -> Dict[str, int]:
        return {"epoch": int(self.epoch), "seed": self.seed}

    def check_state_dict(self, state: Dict[str, int]) -> None:
        if "epoch" not in state or int(state["epoch"]) < 0:
            raise ValueError("batches state: 'epoch' is missing or negative")
        if self.shuffle and int(state.get("seed", self.seed)) != self.seed:
            raise ValueError(f"batches state: 'seed' is {state['seed']}, this object shuffles with {self.seed}")

    def load_state_dict(self, state: Dict[str, int]) -> None:
        self.check_state_dict(state)
        self.epoch = int(state["epoch"])

    def _chunks(self) -> List[np.ndarray]:
        n = len(self.ds)
        order = np.random.RandomState([self.seed, self.epoch]).permutation(n) if self.shuffle else np.arange(n)
        self.epoch += 1
        return [order[i:i + self.bs] for i in range(0, n, self.bs) if not (self.drop_last and i + self.bs > n)]

    def __iter__(self):
        chunks = self._chunks()
        if isinstance(self.ds, Cifar10Binary):
            return ((self.ds.x[idx], self.ds.y[idx]) for idx in chunks)
        return _FolderEpoch(self.ds, chunks, self.workers)


def batches(dataset, batch_size: int, shuffle: bool, seed: int, drop_last: bool = False, num_workers: int = 4) -> _Batches:
    """A re-iterable (with __len__) of HOST batches for ``data.DeviceLoader``; every iteration is one epoch with a fresh
    seeded shuffle.  Cifar10Binary: (uint8 [B,32,32,3], int64 labels).  ImageFolder: (RaggedBatch, int64 labels), decoded
    by min(num_workers, 16) daemon threads, one batch ahead of the consumer."""
    return _Batches(dataset, batch_size, shuffle, seed, drop_last, num_workers)


# ---------------------------------------------------------------- the reference's loader functions ----
def load_cifar10(data_dir: str = "./project/data", img_size: int = 224, batch_size: int = 128, num_workers: int = 4,
                 subset_size: Optional[int] = None, seed: int = 0) -> Dict[str, Any]:
    """Mirror of the reference's load_cifar10 (utils/data_utils.py:83-156); the loaders are DeviceLoaders."""
    tfs = get_transforms("cifar10", img_size, seed=seed)
    train = Cifar10Binary(data_dir, True, subset_size, seed)
    test = Cifar10Binary(data_dir, False, None if subset_size is None else subset_size // 5, seed)
    return {"train_dataset": train, "test_dataset": test,
            "train_loader": DeviceLoader(batches(train, batch_size, True, seed, num_workers=num_workers), tfs["train"]),
            "test_loader": DeviceLoader(batches(test, batch_size, False, seed, num_workers=num_workers), tfs["test"]),
            "class_names": train.classes, "num_classes": len(train.classes)}


def load_imagenet_subset(data_dir: str = "./project/data/imagenet", img_size: int = 224, batch_size: int = 64,
                         num_workers: int = 4, subset_size: Optional[int] = None, seed: int = 0) -> Dict[str, Any]:
    """Mirror of the reference's load_imagenet_subset (utils/data_utils.py:159-244): ImageFolders on train/ and val/.
    num_classes is the number of class directories found (the reference returns the constant 1000)."""
    tfs = get_transforms("imagenet", img_size, seed=seed)
    if not os.path.exists(data_dir):
        raise FileNotFoundError(f"ImageNet directory not found: {data_dir}")
    train_dir, val_dir = os.path.join(data_dir, "train"), os.path.join(data_dir, "val")
    if not os.path.exists(train_dir) or not os.path.exists(val_dir):
        raise FileNotFoundError(f"ImageNet train or validation directory not found in {data_dir}")
    train = ImageFolder(train_dir, subset_size, seed)
    val = ImageFolder(val_dir, None if subset_size is None else subset_size // 5, seed)
    return {"train_dataset": train, "val_dataset": val,
            "train_loader": DeviceLoader(batches(train, batch_size, True, seed, num_workers=num_workers), tfs["train"]),
            "val_loader": DeviceLoader(batches(val, batch_size, False, seed, num_workers=num_workers), tfs["test"]),
            "idx_to_class": {i: c for i, c in enumerate(train.classes)}, "num_classes": len(train.classes)}
