"""Packed uint8 frame store and on-device batch preparation for the two trainers - an opt-in input path beside
data.FrameFolderVideos and lfae_train.FramePairs, which stay the definitions of what a batch is.

    pack_frame_folders(root, out_dir, store_size)      decode every frame of root/<label>/<video>/*.jpg|png ONCE, area-resize it to
                                                       store_size (1, 2 or 4 x the training size) -> frames.u8 + index.json;
                                                       layout="any": every folder of frames at any depth, as FramePairs walks
    PackedVideos(out_dir, image_size, ...)             Dataset over the store: an item is bytes and four jitter numbers, no arithmetic
    DevicePrep(dataset)                                collated batch -> real_vids (B, 3, T, H, W) float32 on the device (ops.video_prep)
    PackedFramePairs(out_dir, frame_shape, ...)        LFAE stage 1: FramePairs' draws over the store, an item is two frames' bytes or rows
    DevicePairPrep(dataset)                            collated batch -> {"source", "driving"} (B, 3, H, W) (ops.frame_pairs_prep)
    pack_latents(model, out_dir, dtype)                the frozen LFAE's flow latent of every stored frame, ONCE -> latents.f32|f16 +
                                                       latents.json
    PackedLatents(out_dir, image_size, ..., model=)    PackedVideos' draws; an item is rows, the reference frame and the latent rows
    DeviceLatentPrep(dataset)                          collated batch -> (latent (B, 3, T, s, s), ref_img (B, 3, H, H))
                                                       (ops.latent_gather, ops.video_prep): FlowDiffusion.set_train_latent's inputs

Colour jitter, the area shrink, the mean and the / 255 run in csrc/video_prep.hip, bit for bit what FrameFolderVideos computes from the
stored bytes.  The approximation is the store itself.  A source larger than store_size is rounded to a byte once, when packed: without
jitter that is at most 0.5 / 255 against the host path on the original files.  With jitter the augmentation then runs at store
resolution, not source resolution (the host jitters the full-size frames and shrinks afterwards); every jitter stage is non-linear, so on
larger originals the two paths are neither bit- nor bound-comparable - several levels of 255 apart on the test's small noisy frames.
"""
import json
import os
import random

import numpy as np
import torch
from torch.utils import data as tdata

from . import _native, ops
from .data import FrameFolderVideos, _rgb, sample_indices
from .lfae_train import FramePairs
from .io_compat import INTER_AREA, imread, resize

FRAMES_FILE, INDEX_FILE = "frames.u8", "index.json"
STORE_VERSION = 1


def _check_sizes(store_size, image_size=None):
    if store_size < 4 or store_size % 4 != 0:
        raise ValueError("store_size must be a multiple of 4, got %r" % (store_size,))
    if image_size is not None:
        if image_size < 4 or image_size % 4 != 0:
            raise ValueError("image_size must be a multiple of 4, got %r" % (image_size,))
        if store_size % image_size != 0 or store_size // image_size not in ops.PREP_RATIOS:
            raise ValueError("store_size / image_size must be 1, 2 or 4 (the shrink factors csrc/video_prep.hip has), got %d / %d"
                             % (store_size, image_size))


def _picture_rect(shape, store_size):
    """Where io_compat.resize puts a frame of `shape` inside the store_size square: (y0, x0, h, w); the rest is zero padding."""
    ratio = float(store_size) / max(shape[:2])
    h, w = (int(x * ratio) for x in shape[:2])
    return [(store_size - h) // 2, (store_size - w) // 2, h, w]


PACK_LAYOUTS = ("label/video", "any")


def _walk_any(root):
    """Every folder under root that holds at least one *.jpg|jpeg|png frame, at any depth, in the order lfae_train.FramePairs walks
    (sorted by folder path) -> [(label, video, paths)]: label is the first path component below root and video the rest of the relative
    path; a folder directly under root (MHAD's and NATOPS' flat layout) has label "" and its own name as video, root itself "" and ""."""
    videos = []
    for folder, _, files in sorted(os.walk(root)):
        frames = sorted(f for f in files if f.lower().endswith(("jpg", "jpeg", "png")))
        if not frames:
            continue
        rel = os.path.relpath(folder, root)
        parts = [] if rel == os.curdir else rel.split(os.sep)
        label, vid = ("", "/".join(parts)) if len(parts) < 2 else (parts[0], "/".join(parts[1:]))
        videos.append((label, vid, [os.path.join(folder, f) for f in frames]))
    if not videos:
        raise FileNotFoundError("no folders with *.jpg|png frames under %r" % (root,))
    return videos


def pack_frame_folders(root, out_dir, store_size, layout="label/video"):
    """Walks root/<label>/<video>/*.jpg|png like FrameFolderVideos - or, layout="any", folders of any depth like lfae_train.FramePairs
    (_walk_any) - and writes out_dir/frames.u8, a flat (N_frames, S, S, 3) uint8 array of
    io_compat.resize(data._rgb(frame), store_size, INTER_AREA) (rounded to a byte, zero-padded to a square), and out_dir/index.json
    (labels, names, first frame, frame count, picture rectangle, store_size).  Returns the index."""
    store_size = int(store_size)
    _check_sizes(store_size)
    if layout not in PACK_LAYOUTS:
        raise ValueError("layout is one of %s, got %r" % (PACK_LAYOUTS, layout))
    videos = FrameFolderVideos(root).videos if layout == "label/video" else _walk_any(root)
    total = sum(len(paths) for _, _, paths in videos)
    os.makedirs(out_dir, exist_ok=True)
    # a raw file, not .npy: np.memmap reads it back with the index's shape
    frames = np.memmap(os.path.join(out_dir, FRAMES_FILE), dtype=np.uint8, mode="w+", shape=(total, store_size, store_size, 3))
    entries, row = [], 0
    for label, vid, paths in videos:
        rect = None
        for k, p in enumerate(paths):
            a = np.ascontiguousarray(_rgb(imread(p)), dtype=np.uint8)
            r = _picture_rect(a.shape, store_size)
            if rect is None:
                rect = r
            elif r != rect:
                raise ValueError("%s: the frames of one video must share a size (frame 0 and frame %d differ)" % (os.path.dirname(p), k))
            frames[row + k] = resize(a, store_size, interpolation=INTER_AREA)
        entries.append({"label": label, "video": vid, "first": row, "count": len(paths), "valid": rect})
        row += len(paths)
    frames.flush()
    del frames
    index = {"version": STORE_VERSION, "store_size": store_size, "frames": total, "videos": entries}
    with open(os.path.join(out_dir, INDEX_FILE), "w") as f:
        json.dump(index, f)
    return index


def draw_jitter(rnd=random, bright=64. / 255, contrast=0.25, sat=0.25, hue=0.04):
    """The four draws of data.color_jitter, same order and ranges -> ((bf, cf, sf) float32, hue shift int(hf * 255))."""
    bf = rnd.uniform(max(0, 1 - bright), 1 + bright)
    cf = rnd.uniform(max(0, 1 - contrast), 1 + contrast)
    sf = rnd.uniform(max(0, 1 - sat), 1 + sat)
    hf = rnd.uniform(-hue, hue)
    return np.array([bf, cf, sf], np.float32), int(hf * 255)


def _open_store(store_dir, image_size):
    """What every data set over a store checks and opens -> (index, store_size, frames memmap (N, S, S, 3))."""
    with open(os.path.join(store_dir, INDEX_FILE)) as f:
        index = json.load(f)
    if index.get("version") != STORE_VERSION:
        raise ValueError("%s: store version %r, this code reads %d" % (store_dir, index.get("version"), STORE_VERSION))
    s = int(index["store_size"])
    _check_sizes(s, image_size)
    if not index["videos"]:
        raise FileNotFoundError("no videos in %r" % (store_dir,))
    # the device shrinks the padded square, the host shrinks the picture and then centres it: the same thing only when the picture
    # starts and ends on a k x k cell
    k = s // image_size
    for v in index["videos"]:
        if any(x % k for x in v["valid"]):
            raise ValueError("%s: video %s/%s has its picture at (y0, x0, h, w) = %s inside the %d x %d stored frame, not on multiples "
                             "of store_size / image_size = %d: a %d x %d cell would mix picture and padding; pack at store_size == "
                             "image_size" % (store_dir, v["label"], v["video"], tuple(v["valid"]), s, s, k, k, k))
    frames = np.memmap(os.path.join(store_dir, FRAMES_FILE), dtype=np.uint8, mode="r", shape=(int(index["frames"]), s, s, 3))
    return index, s, frames


class PackedVideos(tdata.Dataset):
    """Item = (frames uint8 (T, S, S, 3), params float32[3] = (bf, cf, sf), hue_shift int32, label, name, valid int32[4]); with
    resident=True the first entry is the (T,) int32 rows of the store instead of their pixels (DevicePrep holds the store on the
    device).  Frame sampling is data.sample_indices, the jitter draws are data.color_jitter's; jitter=False gives (1, 1, 1), 0 and
    `self.jitter` False, which makes DevicePrep skip the jitter arithmetic altogether (PIL's HSV round trip is lossy even at shift 0)."""

    def __init__(self, store_dir, image_size=128, num_frames=40, sampling="uniform", mean=(0, 0, 0), jitter=False, resident=False):
        self.index, self.store_size, self.frames = _open_store(store_dir, int(image_size))
        self.image_size, self.num_frames, self.sampling, self.jitter, self.resident = int(image_size), num_frames, sampling, jitter, resident
        self.mean = np.asarray(mean, np.float32)
        self.videos = self.index["videos"]

    def __len__(self):
        return len(self.videos)

    def __getitem__(self, index):
        v = self.videos[index]
        rows = v["first"] + sample_indices(v["count"], self.num_frames, self.sampling)
        if self.jitter:
            params, shift = draw_jitter()
        else:
            params, shift = np.ones(3, np.float32), 0
        first = rows.astype(np.int32) if self.resident else np.stack([self.frames[i] for i in rows])
        return first, params, np.array(shift, np.int32), v["label"], "%s_%s" % (v["label"], v["video"]), np.asarray(v["valid"], np.int32)


class _DeviceStore:
    """What DevicePrep and DevicePairPrep share: the device, the resident store (uploaded here, once) and the staging of a batch's bytes
    (_rows_of)."""
    _CHUNK = 1 << 28

    def __init__(self, dataset, device=None):
        self.ds = dataset
        kind = _native.library().kind
        self.device = torch.device(device if device is not None else ("cuda" if kind == "hip" else "cpu"))
        self.cuda = self.device.type == "cuda"
        self._lanes = {}              # lane -> [pinned buffers [2], their copies' events [2], next slot]: one lane per staged operand
        self.store = self._upload(dataset.frames) if dataset.resident else None

    def _upload(self, array):
        """A whole memmap (N, ...) onto the device with its own element type, in pieces of at most _CHUNK bytes."""
        one = torch.from_numpy(np.array(array[:1]))
        dev = torch.empty(tuple(array.shape), dtype=one.dtype, device=self.device)
        step = max(1, self._CHUNK // max(1, one.numel() * one.element_size()))
        for i in range(0, array.shape[0], step):
            dev[i:i + step].copy_(torch.from_numpy(np.array(array[i:i + step])))
        return dev

    def _stage(self, frames, lane=0):
        """(B, T, S, S, 3) uint8 host tensor -> (B * T, S, S, 3) on the device.  lane: which pair of pinned buffers - an operand that is
        staged beside the frames in the same batch takes a lane of its own, so that each keeps two batches in flight."""
        flat = frames.reshape((-1,) + tuple(frames.shape[2:]))
        if not self.cuda:
            return flat.contiguous()
        if flat.is_pinned() and flat.is_contiguous():
            # a DataLoader with pin_memory=True has pinned the collated batch already: no second host copy.  The caching host allocator
            # keeps the block from reuse until this copy has run.
            return flat.to(self.device, non_blocking=True)
        pinned, events, slot = st = self._lanes.setdefault(lane, [[None, None], [None, None], 0])
        k = slot
        st[2] = slot ^ 1
        if events[k] is not None:
            events[k].synchronize()
        if pinned[k] is None or pinned[k].numel() < flat.numel():
            pinned[k] = torch.empty(flat.numel(), dtype=torch.uint8, pin_memory=True)
        host = pinned[k][:flat.numel()].view(flat.shape)
        host.copy_(flat)
        dev = host.to(self.device, non_blocking=True)
        events[k] = torch.cuda.Event()
        events[k].record()
        return dev

    def _rows_of(self, first):
        """A collated batch's first entry - (B, T) rows of the resident store, or (B, T, S, S, 3) bytes - as (store, rows (B, T) int32)."""
        if self.ds.resident:
            return self.store, first.to(torch.int32)
        store = self._stage(first)
        return store, torch.arange(first.shape[0] * first.shape[1], dtype=torch.int32).view(first.shape[0], first.shape[1])


class DevicePrep(_DeviceStore):
    """Callable on a collated PackedVideos batch: returns real_vids (B, 3, T, H, W) float32 on the device; the reference frame is
    real_vids[:, :, 0].  Staged batches cross as bytes through two reused pinned buffers (non_blocking; a buffer is refilled only after
    its last copy has finished); a resident dataset's store is uploaded here, once, and a batch is then a table of row numbers."""

    def __call__(self, batch):
        first, params, shift, valid = batch[0], batch[1], batch[2], batch[5]
        store, rows = self._rows_of(first)
        jitter = bool(self.ds.jitter)
        return ops.video_prep(store, rows, params.to(torch.float32) if jitter else None, shift.to(torch.int32) if jitter else None,
                              self.ds.mean.tolist(), self.ds.image_size, jitter, valid=valid.to(torch.int32) if jitter else None)


class PackedFramePairs(tdata.Dataset):
    """LFAE stage-1 items over a store: lfae_train.FramePairs' draws, in its order and from its sources - the two frame numbers and the
    two flips from FramePairs._generator (one generator per process and DataLoader worker, mixed with `seed`), the four jitter factors
    from `random` with FramePairs' keys and defaults - over the videos of the store that have at least 2 frames, in index order.
    Item = (first, params float32[3], hue_shift int32, flip int32, valid int32[4]): first is the two frames' bytes uint8 (2, S, S, 3),
    or with resident=True their rows int32 (2,) of the store; the time flip has exchanged the two already, the horizontal flip is the
    flag DevicePairPrep hands to the kernel.  No pixel arithmetic.  jitter: None, or the yaml's jitter_param dict."""
    _generator = FramePairs._generator

    def __init__(self, store_dir, frame_shape=128, horizontal_flip=True, time_flip=True, jitter=None, seed=None, resident=False):
        self.index, self.store_size, self.frames = _open_store(store_dir, int(frame_shape))
        self.frame_shape, self.resident = int(frame_shape), resident
        self.horizontal_flip, self.time_flip, self.jitter = horizontal_flip, time_flip, jitter
        self.seed = seed
        self._rng, self._rng_key = None, None
        self.videos = [v for v in self.index["videos"] if v["count"] >= 2]
        if not self.videos:
            raise FileNotFoundError("no videos with >= 2 frames in %r" % (store_dir,))

    def __len__(self):
        return len(self.videos)

    def __getitem__(self, index):
        v = self.videos[index]
        rng = self._generator()
        rows = v["first"] + np.sort(rng.choice(v["count"], size=2, replace=True))
        if self.jitter:
            params, shift = draw_jitter(random, bright=self.jitter.get("brightness", 0.1), contrast=self.jitter.get("contrast", 0.1),
                                        sat=self.jitter.get("saturation", 0.1), hue=self.jitter.get("hue", 0.1))
        else:
            params, shift = np.ones(3, np.float32), 0
        flip = int(bool(self.horizontal_flip and rng.random() < 0.5))
        if self.time_flip and rng.random() < 0.5:
            rows = rows[::-1]
        first = np.ascontiguousarray(rows, np.int32) if self.resident else np.stack([self.frames[i] for i in rows])
        return first, params, np.array(shift, np.int32), np.array(flip, np.int32), np.asarray(v["valid"], np.int32)


class DevicePairPrep(_DeviceStore):
    """Callable on a collated PackedFramePairs batch: returns {"source", "driving"}, (B, 3, H, W) float32 on the device - what
    lfae_train.FramePairs' loader yields.  Staging and the resident store as DevicePrep's."""

    def __call__(self, batch):
        first, params, shift, flip, valid = batch
        store, rows = self._rows_of(first)
        jitter = bool(self.ds.jitter)
        src, drv = ops.frame_pairs_prep(store, rows, params.to(torch.float32) if jitter else None, shift.to(torch.int32) if jitter else None,
                                        flip.to(torch.int32), self.ds.frame_shape, jitter, valid=valid.to(torch.int32) if jitter else None)
        return {"source": src, "driving": drv}


# ---------------------------------------------------------------------------------------------
# the flow-latent store beside frames.u8: the frozen LFAE's outputs of every frame, computed once
# ---------------------------------------------------------------------------------------------
LATENTS_META = "latents.json"
LATENT_FILES = {"f32": "latents.f32", "f16": "latents.f16"}
LATENT_NUMPY = {"f32": np.float32, "f16": np.float16}
LATENT_VERSION = 1


def lfae_fingerprint(model):
    """sha256 (hex) over the frozen LFAE a latent was computed by: the state-dict tensors of model.region_predictor, .bg_predictor and
    .generator in key order (name, dtype, shape, bytes) and model.lfae_config, the yaml's model_params - the switches no weight records
    (temperature, scale factors, pca_based, bg_type, revert_axis_swap, ...).  use_residual_flow is not part of it: the store holds the
    LFAE's raw outputs and serves both settings."""
    import hashlib
    h = hashlib.sha256()
    for name in ("region_predictor", "bg_predictor", "generator"):
        sd = getattr(model, name).state_dict()
        for key in sorted(sd):
            t = sd[key].detach().cpu().contiguous()
            h.update(("%s.%s|%s|%s|" % (name, key, t.dtype, tuple(t.shape))).encode())
            h.update(t.numpy().tobytes())
    h.update(json.dumps(model.lfae_config, sort_keys=True, default=str).encode())
    return h.hexdigest()


def _model_device(model):
    return next(model.unet.parameters()).device


def pack_latents(model, store_dir, dtype="f32", image_size=128, mean=(0, 0, 0), chunk_frames=64):
    """Walks a store written by pack_frame_folders and writes store_dir/latents.f32 (or .f16), a flat (N_frames, 3, S, S) array in the
    frame order of frames.u8 - the frozen LFAE's RAW outputs per frame against frame 0 of its video: sampling grid x, grid y, occlusion
    map (FlowDiffusion._lfae_pass(..., decode=False)), not _latent_of of them, so one store serves use_residual_flow True and False
    and the fp32 store is exact for both (ops.latent_gather applies _latent_of) - and store_dir/latents.json (version, dtype, S,
    image_size, mean, frame count, lfae_fingerprint).  Every video's frames reach the device through the un-jittered ops.video_prep path.
    A video with count <= chunk_frames goes through ONE pass with B = 1, nf = count: its stored fp32 latent is bit for bit what
    model.encode_video returns for the same prepared frames.  A longer video goes in chunks of chunk_frames frames; the kernels' launch
    plans depend on the row count, so a chunked result is only close to the one-pass result (within the suite's 1e-3 parity bar), not
    equal to it.  fp16 rounds each value once (at most half an fp16 ulp: 2^-12 for |v| < 1).  Returns the meta dict."""
    if dtype not in LATENT_FILES:
        raise ValueError("dtype is one of %s, got %r" % (tuple(LATENT_FILES), dtype))
    chunk_frames, image_size = int(chunk_frames), int(image_size)
    if chunk_frames < 1:
        raise ValueError("chunk_frames must be at least 1, got %d" % chunk_frames)
    index, _, frames = _open_store(store_dir, image_size)
    mean = [float(m) for m in mean]
    dev = _model_device(model)
    n, out, s = int(index["frames"]), None, None
    for v in index["videos"]:
        first, count, ref = int(v["first"]), int(v["count"]), None
        for c0 in range(0, count, chunk_frames):
            k = min(chunk_frames, count - c0)
            store = torch.from_numpy(np.array(frames[first + c0:first + c0 + k])).to(dev)
            vid = ops.video_prep(store, torch.arange(k, dtype=torch.int32).view(1, k), None, None, mean, image_size, False)
            if ref is None:
                ref = vid[:, :, 0].clone()
            g = model._lfae_pass(vid, ref, False)
            raw = torch.cat((g["optical_flow"], g["occlusion_map"]), dim=1)[0].permute(1, 0, 2, 3)          # (k, 3, S, S)
            if out is None:
                s = int(raw.shape[-1])
                if tuple(raw.shape[1:]) != (3, s, s):
                    raise ValueError("the LFAE returned maps of shape %s, expected (3, S, S)" % (tuple(raw.shape[1:]),))
                out = np.memmap(os.path.join(store_dir, LATENT_FILES[dtype]), dtype=LATENT_NUMPY[dtype], mode="w+", shape=(n, 3, s, s))
            out[first + c0:first + c0 + k] = raw.to(torch.float16 if dtype == "f16" else torch.float32).cpu().numpy()
    out.flush()
    del out
    meta = {"version": LATENT_VERSION, "dtype": dtype, "latent_size": s, "image_size": image_size, "mean": mean, "frames": n,
            "chunk_frames": chunk_frames, "fingerprint": lfae_fingerprint(model)}
    with open(os.path.join(store_dir, LATENTS_META), "w") as f:
        json.dump(meta, f)
    return meta


class PackedLatents(tdata.Dataset):
    """Dataset over a store with a latent store beside it (pack_latents), next to PackedVideos: the same draws in the same order -
    data.sample_indices, then draw_jitter - but an item carries no video: (rows int32 (T,) of the store, ref, latent, params float32[3],
    hue_shift int32, label, name, valid int32[4]).  ref is the REFERENCE frame only, rows[0] == the video's first frame: its bytes
    uint8 (1, S, S, 3), or with resident=True its row int32 (1,).  latent is the T latent rows from the memmap (T, 3, s, s) float32 /
    float16, or with resident=True an empty array (DeviceLatentPrep holds both stores on the device).
    model: the FlowDiffusion that will train (its LFAE is fingerprinted), or fingerprint=: a lfae_fingerprint string.  A store whose
    fingerprint, latent size, image_size or mean differ is refused: a latent computed by another LFAE, or from other pixels, is silently
    wrong otherwise.  residual: use_residual_flow of the consumer (default: the model's).
    The one approximation: with jitter=True the online path jitters the whole video before the LFAE sees it; here the
    flows are those of the un-jittered frames and only the reference frame - and so ref_img_fea - is jittered."""

    def __init__(self, store_dir, image_size=128, num_frames=40, sampling="uniform", mean=(0, 0, 0), jitter=False, resident=False, *,
                 model=None, fingerprint=None, residual=None):
        if (model is None) == (fingerprint is None):
            raise ValueError("PackedLatents: give the model that will train, or the fingerprint of its LFAE (exactly one of the two)")
        self.index, self.store_size, self.frames = _open_store(store_dir, int(image_size))
        self.image_size, self.num_frames, self.sampling, self.jitter, self.resident = int(image_size), num_frames, sampling, jitter, resident
        self.mean = np.asarray(mean, np.float32)
        self.videos = self.index["videos"]
        meta_path = os.path.join(store_dir, LATENTS_META)
        if not os.path.exists(meta_path):
            raise FileNotFoundError("%s: no %s - build the latent store with tools/pack_latents.py" % (store_dir, LATENTS_META))
        with open(meta_path) as f:
            self.meta = meta = json.load(f)
        if meta.get("version") != LATENT_VERSION or meta.get("dtype") not in LATENT_FILES:
            raise ValueError("%s: latent store version %r / dtype %r, this code reads version %d and %s"
                             % (store_dir, meta.get("version"), meta.get("dtype"), LATENT_VERSION, tuple(LATENT_FILES)))
        want = lfae_fingerprint(model) if model is not None else str(fingerprint)
        if meta["fingerprint"] != want:
            raise ValueError("%s: the latent store was computed by another LFAE (fingerprint %s..., this model's is %s...): pack it "
                             "again with this model's checkpoint and config" % (store_dir, meta["fingerprint"][:12], want[:12]))
        self.latent_size = int(meta["latent_size"])
        if model is not None and self.latent_size != int(model.diffusion.image_size):
            raise ValueError("%s: latents of %d x %d, the model denoises %d x %d" % (store_dir, self.latent_size, self.latent_size,
                                                                                     model.diffusion.image_size, model.diffusion.image_size))
        if int(meta["image_size"]) != self.image_size or [float(m) for m in meta["mean"]] != [float(m) for m in self.mean]:
            raise ValueError("%s: latents packed at image_size %s and mean %s, asked for %d and %s"
                             % (store_dir, meta["image_size"], meta["mean"], self.image_size, self.mean.tolist()))
        if int(meta["frames"]) != int(self.index["frames"]):
            raise ValueError("%s: %s latent rows for %s frames: the frame store was packed again" % (store_dir, meta["frames"], self.index["frames"]))
        self.residual = bool(model.use_residual_flow if residual is None and model is not None else residual)
        self.dtype = meta["dtype"]
        self.latents = np.memmap(os.path.join(store_dir, LATENT_FILES[self.dtype]), dtype=LATENT_NUMPY[self.dtype], mode="r",
                                 shape=(int(meta["frames"]), 3, self.latent_size, self.latent_size))

    def __len__(self):
        return len(self.videos)

    def __getitem__(self, index):
        v = self.videos[index]
        rows = v["first"] + sample_indices(v["count"], self.num_frames, self.sampling)
        if self.jitter:
            params, shift = draw_jitter()
        else:
            params, shift = np.ones(3, np.float32), 0
        assert rows[0] == v["first"], "the latents are relative to frame 0 of the video: sample_indices must start there"
        rows = rows.astype(np.int32)
        if self.resident:
            ref, latent = rows[:1].copy(), np.zeros((0,), LATENT_NUMPY[self.dtype])
        else:
            ref, latent = np.array(self.frames[rows[0]:rows[0] + 1]), np.stack([self.latents[i] for i in rows])
        return rows, ref, latent, params, np.array(shift, np.int32), v["label"], "%s_%s" % (v["label"], v["video"]), np.asarray(v["valid"], np.int32)


class DeviceLatentPrep(_DeviceStore):
    """Callable on a collated PackedLatents batch: returns (latent (B, 3, T, s, s), ref_img (B, 3, H, H)) float32 on the device - the
    inputs of FlowDiffusion.set_train_latent.  latent is ops.latent_gather of the batch's rows (the space encode_video returns);
    ref_img is ops.video_prep on the (B, 1) table of reference rows with the item's jitter, so it is torch.equal to
    DevicePrep(...)[:, :, 0] under the same draws.  Resident: both stores are uploaded here, once.  Staged: the reference frames and the
    latent rows (as a uint8 view) cross through two pinned buffers each.  labels and names are batch[5], batch[6]."""

    def __init__(self, dataset, device=None):
        super().__init__(dataset, device)
        self.latents = self._upload(dataset.latents) if dataset.resident else None

    def _prep(self, store, rows, batch):
        params, shift, valid, jitter = batch[3], batch[4], batch[7], bool(self.ds.jitter)
        return ops.video_prep(store, rows, params.to(torch.float32) if jitter else None, shift.to(torch.int32) if jitter else None,
                              self.ds.mean.tolist(), self.ds.image_size, jitter, valid=valid.to(torch.int32) if jitter else None)

    def __call__(self, batch):
        rows, ref, lat = batch[0], batch[1], batch[2]
        b, t = int(rows.shape[0]), int(rows.shape[1])
        if self.ds.resident:
            frames, ref_rows, latents, lat_rows = self.store, ref.to(torch.int32), self.latents, rows.to(torch.int32)
        else:
            frames, ref_rows = self._stage(ref), torch.arange(b, dtype=torch.int32).view(b, 1)
            latents = self._stage(lat.contiguous().view(torch.uint8), lane=1).view(lat.dtype)
            lat_rows = torch.arange(b * t, dtype=torch.int32).view(b, t)
        ref_img = self._prep(frames, ref_rows, batch)[:, :, 0]
        return ops.latent_gather(latents, lat_rows, self.ds.residual), ref_img

    def real_frames(self, batch):
        """The batch's real video (B, 3, T, H, H), what DevicePrep returns for the same draws - for FlowDiffusion.decode_step_logs, at the
        trainer's --save-img-freq only: from the resident store, or from the rows' bytes read from the memmap here."""
        rows = batch[0]
        if self.ds.resident:
            return self._prep(self.store, rows.to(torch.int32), batch)
        b, t = int(rows.shape[0]), int(rows.shape[1])
        host = torch.from_numpy(np.stack([self.ds.frames[int(i)] for i in rows.reshape(-1)]))
        return self._prep(host.to(self.device), torch.arange(b * t, dtype=torch.int32).view(b, t), batch)
