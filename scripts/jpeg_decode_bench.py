"""GPU box: the device JPEG decoder (csrc/jpeg_decode.hip) against Pillow's on one core, on the bench batch of
profiles/jpeg_decode_notes.md: 12 picture-like 375 x 1242 frames (scripts/jpeg_bench.py's `photo`) written by Pillow at quality 95, 4:2:0.

    python scripts/jpeg_decode_bench.py [--rounds 5] [--iters 20] [--photos 24]

One JSON line:
  sweep           per subseq_bits 128 .. 2048: `launches` the most sync launches a file of the batch needed to settle (the kernels' own
                  counter), `hops` the most hops a workgroup looped in one launch, `decode_us` fp_jpeg_decode alone between HIP events
                  with max_rounds = 2 x launches, scans already on the device -- median / min / max over the rounds
  default         the same at ops.JPEG_DECODE_SUBSEQ_BITS / JPEG_DECODE_MAX_ROUNDS
  call_ms         parse + pack on the host, upload, decode, the status back (waits); pack_ms the host part alone
  pillow_ms       Image.open(f).convert("RGB") of the same 12 files on one core
  uploaded_bytes  scans + records + tables against the decoded pixels
  predict_simple_ms_per_image   a folder of --photos such files, --device_resize --device_vis --device_jpeg --batch_size 12, with and
                  without --device_decode, alternating in the same run
Kernel durations are NOT in here: they need a trace of their own."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import _lib, ops

B = 12


def photo(h, w, seed):
    """scripts/jpeg_bench.py's picture-like frame: sky-to-ground shading, a few flat shapes, mild sensor noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([90 + 100 * yy / h + 20 * np.sin(xx / 97), 110 + 60 * yy / h + 25 * np.cos(xx / 61), 160 - 70 * yy / h + 15 * np.sin((xx + yy) / 45)], -1)
    for _ in range(12):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(10, 90)
        inside = (yy - cy) ** 2 + ((xx - cx) / 2) ** 2 < r * r
        img[inside] = img[inside] * 0.4 + rng.uniform(0, 255, 3) * 0.6
    return np.clip(img + rng.normal(0, 2.5, img.shape), 0, 255).astype(np.uint8)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(values, digits=2):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


class Resident:
    """the batch's scans, records and tables on the device: fp_jpeg_decode alone"""

    def __init__(self, pack):
        self.pack = pack
        self.scans = torch.from_numpy(pack["scans"]).cuda()
        self.rec = torch.from_numpy(pack["records"]).cuda()
        self.tab = torch.from_numpy(pack["tables"].view("int32")).cuda()
        self.out = torch.empty(pack["out_bytes"], dtype=torch.uint8, device="cuda")
        self.status = torch.empty(pack["B"] + 1, dtype=torch.int32, device="cuda")

    def launch(self, bits, rounds):
        p, lib = self.pack, _lib.load()
        need = lib.fp_jpeg_decode_workspace_bytes(p["B"], p["max_h"], p["max_w"], p["max_scan"], bits)
        ws = ops.workspace(need, self.out.device, "jpeg_decode")
        _lib.check(lib.fp_jpeg_decode(self.scans.data_ptr(), p["scan_bytes"], self.rec.data_ptr(), self.tab.data_ptr(), p["n_sets"], self.out.data_ptr(),
                                      self.out.numel(), self.status.data_ptr(), p["B"], p["max_h"], p["max_w"], p["max_scan"], bits, rounds,
                                      ws.data_ptr(), ws.numel(), ops.stream()), "fp_jpeg_decode")
        return ws

    def measure(self, bits, rounds, iters, repeats):
        self.launch(bits, rounds)
        torch.cuda.synchronize()
        us = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                self.launch(bits, rounds)
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / iters)
        return spread(us, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photos", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench needs a MI355X: a timing taken elsewhere says nothing")
    from PIL import Image, features
    frames = [photo(375, 1242, 80 + i) for i in range(B)]
    files = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="JPEG", quality=95)
        files.append(buf.getvalue())
    pillow = lambda: [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
    want = pillow()
    result = {"bench": "jpeg_decode", "B": B, "rounds": args.rounds, "iters": args.iters, "libjpeg_turbo": bool(features.check_feature("libjpeg_turbo")),
              "file_bytes": sum(len(f) for f in files)}
    pack = ops.jpeg_decode_pack(files)
    res = Resident(pack)
    sweep = {}
    for bits in (128, 256, 512, 1024, 2048):
        ws = res.launch(bits, 64)
        info = ws[:B * 32].view(torch.int32).view(B, 8).cpu().numpy()
        assert res.status.cpu().tolist() == [0] * (B + 1), res.status.cpu().tolist()
        launches = int(info[:, 1].max()) + 1
        sweep[bits] = {"launches": launches, "hops": int(info[:, 2].max()), "decode_us": res.measure(bits, 2 * launches, args.iters, args.rounds)}
    result["sweep"] = sweep
    result["default"] = {"subseq_bits": ops.JPEG_DECODE_SUBSEQ_BITS, "max_rounds": ops.JPEG_DECODE_MAX_ROUNDS,
                         "decode_us": res.measure(ops.JPEG_DECODE_SUBSEQ_BITS, ops.JPEG_DECODE_MAX_ROUNDS, args.iters, args.rounds)}
    got = ops.jpeg_decode(files, return_status=True)
    result["equal_to_pillow"] = bool(got[1] == [0] * B and all(np.array_equal(a, w) for a, w in zip(got[0], want)))

    def call():
        p = ops.jpeg_decode_pack(files)
        return ops.jpeg_decode_packed(p)[2].cpu()
    call()
    result["call_ms"] = spread([wall(call) * 1e3 for _ in range(args.rounds)])
    result["pack_ms"] = spread([wall(lambda: ops.jpeg_decode_pack(files)) * 1e3 for _ in range(args.rounds)])
    result["pillow_ms"] = spread([wall(pillow) * 1e3 for _ in range(args.rounds)])
    result["uploaded_bytes"] = {"device_decode": int(pack["scan_bytes"] + pack["records"].size + pack["tables"].size * 4), "host_decode": int(pack["out_bytes"])}

    # ---- folder prediction
    from footprints_amd.model_manager import ModelManager
    from footprints_amd.predict_simple import InferenceManager
    torch.manual_seed(5)
    mm = ModelManager(is_inference=True)
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "photos")
        os.makedirs(folder)
        for i in range(args.photos):
            with open(os.path.join(folder, "%04d.jpg" % i), "wb") as fh:
                fh.write(files[i % B])
        managers = {k: InferenceManager("kitti", os.path.join(tmp, k), model_manager=mm, device_resize=True, device_vis=True, batch_size=B,
                                        device_jpeg=True, device_decode=(k == "device_decode")) for k in ("host_decode", "device_decode")}
        ms = {k: [] for k in managers}
        with contextlib.redirect_stdout(io.StringIO()):
            for m in managers.values():
                m.predict(folder)
            for _ in range(args.rounds):
                for k, m in managers.items():
                    ms[k].append(wall(lambda: m.predict(folder)) * 1e3 / args.photos)
        result["predict_simple_ms_per_image"] = {k: spread(v, 3) for k, v in ms.items()}
        same = lambda sub: all(open(os.path.join(tmp, "host_decode", sub, f), "rb").read() == open(os.path.join(tmp, "device_decode", sub, f), "rb").read()
                               for f in sorted(os.listdir(os.path.join(tmp, "host_decode", sub))))
        result["predict_simple_files_equal"] = bool(same("outputs") and same("visualisations"))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
