"""File readers of the training-label generators (reference preprocessing/ground_truth_generation/data_loader.py): KITTILoader and
MatterportLoader with the reference's constructor arguments, attributes and file layout, np.load and Pillow only.

The host reads and plans; everything behind the file runs on the device (csrc/gt_frames.hip).  A loader keeps every frame it has read in a
device-resident cache of float32 [H, W] slots (FrameCache): the frames a call misses go up in ONE packed buffer at their native sizes and
stored dtypes and are resized by ONE launch (cv2.resize's INTER_LINEAR / INTER_NEAREST on float64, the `disp *= width / w` in the stored dtype,
the threshold, the flow's scale, the rounding to float32); a target frame's batch is a gather of cache slots (`depths = fx * baseline /
disparity` in float32 there).  Consecutive KITTI target frames share all but two to four source frames, so a warm call uploads only those.

What the loaders return is what ground_truth_generator's docstring promises; the maps are float32 device tensors that VIEW cache slots:
they stay valid until the loader's next purge (buffered frames) or its next unbuffered load (`use_buffer=False`, Matterport's
`load_frame_data`).  Poses and intrinsics stay on the host."""
import os

import numpy as np
import torch

from ... import ops


class FrameCache:
    """float32 [slots, H, W] on the device plus the pinned staging buffer of its uploads.  Slots are handed out in order and freed all at
    once (`reset`); the cache doubles when it is full, keeping what it holds."""

    def __init__(self, height, width, device=None, slots=160):
        if not torch.cuda.is_available():
            raise RuntimeError("footprints_amd.preprocessing.ground_truth_generation: needs a GPU (no CPU path in the product)")
        self.H, self.W = int(height), int(width)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.tables = ops.linear_table_set(self.device)
        self.first_slots = int(slots)
        self.cache, self.used = None, 0
        self.h_packed, self.copied = None, None
        self.uploads = []                     # (maps, bytes) of every upload since the last reset

    def alloc(self, n):
        """n consecutive free slots"""
        need = self.used + n
        if self.cache is None or need > self.cache.shape[0]:
            cap = max(self.first_slots, need, 0 if self.cache is None else 2 * self.cache.shape[0])
            grown = torch.empty((cap, self.H, self.W), dtype=torch.float32, device=self.device)
            if self.used:
                grown[:self.used].copy_(self.cache[:self.used])
            ops.release(self.cache, "gt frame cache")
            self.cache = grown
        first, self.used = self.used, need
        return list(range(first, need))

    def reset(self):
        self.used = 0
        self.uploads.clear()

    def view(self, slot, n=None):
        """slot as [H, W], or the n slots from `slot` on as [n, H, W]"""
        return self.cache[slot] if n is None else self.cache[slot:slot + n]

    def resize_into(self, maps, slots, method="linear", pre=1.0, post=1.0, threshold=None):
        """maps (native size, stored dtype) -> their slots: one packed upload, one launch"""
        need = ops.gt_frame_pack_bytes(maps)
        if self.copied is not None:
            self.copied.synchronize()         # the previous upload still reads the staging buffer
        if self.h_packed is None or self.h_packed.numel() < need:
            self.h_packed = torch.empty(max(need, 1 << 20), dtype=torch.uint8).pin_memory()
        hw = self.H * self.W
        pack = ops.gt_frame_pack(maps, self.H, self.W, [s * hw for s in slots], self.cache.numel(), method, pre, post, threshold, self.tables,
                                 packed=self.h_packed.numpy())
        d_packed = torch.empty(pack.total, dtype=torch.uint8, device=self.device)
        d_packed.copy_(self.h_packed[:pack.total], non_blocking=True)
        self.copied = torch.cuda.Event()
        self.copied.record()
        ops.gt_frame_resize(pack, d_packed, self.cache)
        self.uploads.append((len(maps), pack.total))

    def gather(self, depth_slots, seg_slots, fb=None):
        return ops.gt_gather_frames(self.cache, depth_slots, seg_slots, fb)


class BaseLoader:
    """what the two loaders share: the folders, the target size, the threshold and the frame cache (made at the first load)"""

    def __init__(self, raw_data_path, training_data_path, height, width, footprint_threshold=0.75, frame_cache=None):
        self.raw_data_path = raw_data_path
        self.training_data_path = training_data_path
        self.height = height
        self.width = width
        self.footprint_threshold = footprint_threshold
        self._cache = frame_cache
        self._scratch = None                  # the slots of unbuffered loads

    @property
    def frame_cache(self):
        if self._cache is None:
            self._cache = FrameCache(self.height, self.width)
        return self._cache

    def _scratch_slots(self, n):
        if self._scratch is None or len(self._scratch) < n:
            self._scratch = self.frame_cache.alloc(n)
        return self._scratch[:n]

    def _free_slots(self):
        if self._cache is not None:
            self._cache.reset()
        self._scratch = None

    def load_data(self):
        raise NotImplementedError

    def load_frame_data(self):
        raise NotImplementedError


class KITTILoader(BaseLoader):
    """Frames for the KITTI generators.  `load_data` returns the window of source frames around a target frame (every second frame from
    num_frames_bwd before to num_frames_fwd after it, both cameras); `buffer` maps (sequence, int(frame), side) to the frame's pose and
    cache slots, so a frame is read, uploaded and resized once however many windows it lies in."""

    SIDES = ("image_02", "image_03")

    def __init__(self, raw_data_path, training_data_path, height, width, num_frames_bwd=25, num_frames_fwd=50, footprint_threshold=0.75,
                 frame_cache=None):
        super().__init__(raw_data_path, training_data_path, height, width, footprint_threshold=footprint_threshold, frame_cache=frame_cache)
        self.num_frames_bwd = num_frames_bwd
        self.num_frames_fwd = num_frames_fwd
        self.buffer = {}
        self.K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        self.K[0] *= width
        self.K[1] *= height
        self.invK = np.linalg.pinv(self.K)
        self.stereo_baseline = 0.54

    # ---- files
    def _path(self, *parts):
        return os.path.join(self.training_data_path, *parts)

    def _read_flow(self, sequence, frame, side):
        return np.load(self._path("optical_flow", sequence, side, "data", "{}.npy".format(str(frame).zfill(10))))

    def _read(self, sequence, frame, side, load_flow):
        """the files of one frame as np.load returns them, or None when one is missing (a frame outside the sequence)"""
        name = "{}.npy".format(str(frame).zfill(10))
        try:
            raw = {"disparity": np.load(self._path("stereo_matching_disps", sequence, side, name)),
                   "ground_seg": np.load(self._path("ground_seg", sequence, side, "data", name))[0]}
            pose = np.eye(4)
            pose[:3] = np.load(self._path("poses", sequence, "orbslam_poses", name)).reshape(3, 4)
            raw["pose"] = pose
            if load_flow:
                raw["flow"] = self._read_flow(sequence, frame, side)
        except FileNotFoundError:
            return None
        return raw

    # ---- the plan of one upload
    def _flow_records(self, flow):
        return [(flow[0], 1.0, (float(self.width), float(flow.shape[2])), None), (flow[1], 1.0, (float(self.height), float(flow.shape[1])), None)]

    def _records(self, raw, threshold_ground):
        """(map, pre, post, threshold) of one frame's maps in slot order: disparity, ground segmentation, flow x and y"""
        disp = raw["disparity"]
        rec = [(disp, self.width / disp.shape[1], 1.0, None),
               (raw["ground_seg"], 1.0, 1.0, self.footprint_threshold if threshold_ground else None)]
        return rec + (self._flow_records(raw["flow"]) if "flow" in raw else [])

    def _resize(self, records, slots):
        self.frame_cache.resize_into([r[0] for r in records], slots, "linear", [r[1] for r in records], [r[2] for r in records],
                                     [r[3] for r in records])

    def _insert(self, frames, threshold_ground=True):
        """frames: [(key, raw)] -> one upload and one launch for all of them; the entries go into the buffer"""
        records, entries = [], []
        for key, raw in frames:
            rec = self._records(raw, threshold_ground)
            entries.append((key, raw["pose"], len(records), len(rec)))
            records += rec
        slots = self.frame_cache.alloc(len(records))
        self._resize(records, slots)
        for key, pose, first, n in entries:
            entry = {"pose": pose, "disparity": slots[first], "ground_seg": slots[first + 1]}
            if n == 4:
                entry["flow"] = slots[first + 2]
            self.buffer[key] = entry

    def _data(self, entry):
        """a frame as the generators take it: the maps are views of the frame's cache slots"""
        c = self.frame_cache
        data = {"pose": entry["pose"], "disparity": c.view(entry["disparity"]), "ground_seg": c.view(entry["ground_seg"])}
        if "flow" in entry:
            data["flow"] = c.view(entry["flow"], 2)
        return data

    # ---- the reference's interface
    def window(self, frame):
        """the (frame, side) pairs that are projected into `frame`, in the reference's order"""
        return [(f, s) for f in range(frame - self.num_frames_bwd, frame + self.num_frames_fwd, 2) for s in self.SIDES]

    def load_data(self, sequence, frame):
        """depths, ground segmentations (device, [B, H, W]), poses, sides and intrinsics (host) of the frames projected into `frame`"""
        keys = [(sequence, f, s) for f, s in self.window(int(frame))]
        misses = []
        for key in keys:
            if key not in self.buffer and key[1] >= 0:
                raw = self._read(sequence, key[1], key[2], False)
                if raw is not None:
                    misses.append((key, raw))
        if misses:
            self._insert(misses)
        present = [self.buffer[key] for key in keys if key in self.buffer]
        if not present:
            raise ValueError("footprints_amd KITTILoader: no frame of %s around frame %d exists" % (sequence, int(frame)))
        fb = np.float32(float(self.K[0, 0]) * self.stereo_baseline)
        depths, ground_segs = self.frame_cache.gather([e["disparity"] for e in present], [e["ground_seg"] for e in present], float(fb))
        B = len(present)
        return {"depths": depths, "ground_segs": ground_segs,
                "poses": torch.from_numpy(np.stack([e["pose"] for e in present])).float(),
                "sides": [key[2] for key in keys if key in self.buffer],
                "intrinsics": torch.from_numpy(np.stack([self.K] * B)).float(),
                "inv_intrinsics": torch.from_numpy(np.stack([self.invK] * B)).float()}

    def load_frame_data(self, sequence, frame, side, load_flow=False, use_buffer=True, threshold_ground=True):
        """pose, disparity and ground segmentation of one frame, and its flow with `load_flow`; None for a frame with a file missing.
        `use_buffer=False` reads the files again into slots of its own and leaves the buffer alone."""
        key = (sequence, int(frame), side)
        if use_buffer:
            entry = self.buffer.get(key)
            if entry is not None and load_flow and "flow" not in entry:          # buffered by a window, now asked for its flow
                try:
                    flow = self._read_flow(sequence, key[1], side)
                except FileNotFoundError:
                    return None
                slots = self.frame_cache.alloc(2)
                self._resize(self._flow_records(flow), slots)
                entry["flow"] = slots[0]
            if entry is not None:
                return self._data(entry)
        raw = self._read(sequence, key[1], side, load_flow) if key[1] >= 0 else None
        if raw is None:
            return None
        if use_buffer:
            self._insert([(key, raw)], threshold_ground)
            return self._data(self.buffer[key])
        records = self._records(raw, threshold_ground)
        slots = self._scratch_slots(4)[:len(records)]
        self._resize(records, slots)
        entry = {"pose": raw["pose"], "disparity": slots[0], "ground_seg": slots[1]}
        if len(records) == 4:
            entry["flow"] = slots[2]
        return self._data(entry)

    def purge_buffer(self):
        """forget every frame and free every slot"""
        self.buffer = {}
        self._free_slots()


class MatterportLoader(BaseLoader):
    """Frames for the Matterport generators: `load_data` loads a whole scan at once (every frame with a ground segmentation), and the
    generator projects the frames whose cameras are close to the target's.  `scan_data` holds the scan's depths and ground segmentations
    as device tensors that view the cache; `gather_frames` selects frames by index."""

    CHUNK = 32                                # frames per upload: 32 x (480 x 640 uint16 + a segmentation) stay within ~50 MB of pinned memory

    def __init__(self, raw_data_path, training_data_path, height, width, footprint_threshold=0.75, frame_cache=None):
        super().__init__(raw_data_path, training_data_path, height, width, footprint_threshold=footprint_threshold, frame_cache=frame_cache)
        self.current_scan = None
        self.scan_data = None
        self.pose_tracker = {}
        self.full_size_width = 1280.0
        self.full_size_height = 1024.0
        self._scan_slots = (0, 0)             # first depth slot and frame count of the scan in the cache

    def _read(self, scan, pos, height, direction):
        """one frame's files: the stored ground segmentation, the depth PNG resized by Pillow's NEAREST (uint16), pose and intrinsics"""
        from PIL import Image
        scan_path = os.path.join(self.raw_data_path, scan, scan)
        seg = np.load(os.path.join(self.training_data_path, "ground_seg", scan, "data", "{}_{}_{}.npy".format(pos, height, direction)))[0]
        with Image.open(os.path.join(scan_path, "matterport_depth_images", "{}_d{}_{}.png".format(pos, height, direction))) as im:
            depth = np.array(im.resize((self.width, self.height), resample=Image.NEAREST))
        if depth.dtype != np.uint16:
            if depth.min() < 0 or depth.max() > 65535:
                raise ValueError("footprints_amd MatterportLoader: %s %s_d%s_%s.png is not a 16-bit depth image" % (scan, pos, height, direction))
            depth = depth.astype(np.uint16)
        with open(os.path.join(scan_path, "matterport_camera_poses", "{}_pose_{}_{}.txt".format(pos, height, direction))) as fh:
            pose = np.array(fh.read().split()).astype(float).reshape(4, 4)
        K = np.eye(4)
        with open(os.path.join(scan_path, "matterport_camera_intrinsics", "{}_intrinsics_{}.txt".format(pos, height))) as fh:
            words = fh.read().split()
        K[0, 0], K[0, 2], K[1, 1], K[1, 2] = float(words[2]), float(words[4]), float(words[3]), float(words[5])
        K[0] *= self.width / self.full_size_width
        K[1] *= self.height / self.full_size_height
        return seg, depth, pose, K

    def _seg_threshold(self, seg):
        """the reference compares in the stored dtype (`np.load(...)[0] > threshold`): numpy rounds the threshold to that dtype first"""
        return float(seg.dtype.type(self.footprint_threshold)) if seg.dtype.kind == "f" else float(self.footprint_threshold)

    def _resize(self, frames, depth_slots, seg_slots):
        """[(seg, depth)] -> slots: the segmentation through nearest + threshold (equal to threshold, then NEAREST: the values are 0 / 1),
        the depth through a same-size nearest with the 0.00025 metres per unit"""
        maps = [d for _, d in frames] + [s for s, _ in frames]
        n = len(frames)
        self.frame_cache.resize_into(maps, list(depth_slots) + list(seg_slots), "nearest", 1.0, [0.00025] * n + [1.0] * n,
                                     [None] * n + [self._seg_threshold(s) for s, _ in frames])

    def load_data(self, scan, pos, height, direction):
        if self.current_scan != scan:
            self.pose_tracker = {}
            self.current_scan = scan
            self.load_scan_data()
        return dict(self.scan_data)

    def load_frame_data(self, scan, pos, height, direction, threshold_ground=True):
        """-> (ground_seg, depth, pose, K) of one frame; the two maps are views of two slots that the next call overwrites"""
        seg, depth, pose, K = self._read(scan, pos, height, direction)
        slots = self._scratch_slots(2)
        self._resize([(seg, depth)], slots[:1], slots[1:])
        return self.frame_cache.view(slots[1]), self.frame_cache.view(slots[0]), pose, K

    def load_scan_data(self):
        """every frame of the current scan into the cache; poses and intrinsics on the host"""
        folder = os.path.join(self.training_data_path, "ground_seg", self.current_scan, "data")
        names = []
        for file in sorted(os.listdir(folder)):
            if file[-4:] == ".npy" and file[0] != ".":
                pos, height, direction = file.split("_")
                names.append((pos, height, direction[0]))              # the direction carries the extension
        if not names:
            raise ValueError("footprints_amd MatterportLoader: %s holds no ground segmentation" % folder)
        self._free_slots()
        n = len(names)
        self._scratch_slots(2)                # in front of the scan: load_frame_data never makes the cache grow under scan_data's views
        first = self.frame_cache.alloc(2 * n)[0]
        poses, intrinsics, inv_intrinsics = [], [], []
        for c0 in range(0, n, self.CHUNK):
            frames = []
            for pos, height, direction in names[c0:c0 + self.CHUNK]:
                seg, depth, pose, K = self._read(self.current_scan, pos, height, direction)
                frames.append((seg, depth))
                poses.append(pose)
                intrinsics.append(K)
                inv_intrinsics.append(np.linalg.pinv(K))
                self.pose_tracker[(pos, height, direction)] = pose
            self._resize(frames, range(first + c0, first + c0 + len(frames)), range(first + n + c0, first + n + c0 + len(frames)))
        self._scan_slots = (first, n)
        self.scan_data = {"depths": self.frame_cache.view(first, n), "ground_segs": self.frame_cache.view(first + n, n),
                          "poses": torch.from_numpy(np.stack(poses)).float(),
                          "intrinsics": torch.from_numpy(np.stack(intrinsics)).float(),
                          "inv_intrinsics": torch.from_numpy(np.stack(inv_intrinsics)).float()}

    def gather_frames(self, indices):
        """(depths, ground_segs) [len(indices), H, W] of the scan's frames `indices`, gathered out of the cache"""
        first, n = self._scan_slots
        indices = [int(i) for i in indices]
        if any(i < 0 or i >= n for i in indices):
            raise ValueError("footprints_amd MatterportLoader: frame index outside the scan's %d frames" % n)
        return self.frame_cache.gather([first + i for i in indices], [first + n + i for i in indices], None)
