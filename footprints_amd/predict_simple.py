"""predict_simple -- drop-in CLI of footprints/predict_simple.py:29-141 on the HIP engine.

    python -m footprints_amd.predict_simple --image P --model {kitti,matterport,handheld}
                                            [--no_save_vis] [--save_dir D] [--weights W]

Same artefacts as the reference: <save_dir>/outputs/<stem>.npy = float32 [4,H,W] (channels 0,1 LOGITS,
2,3 sigmoid disparities, predict_simple.py:67-73) and <save_dir>/visualisations/<stem>.jpg.  Host plumbing is
restated without the libraries this image lacks: torchvision's Resize(ANTIALIAS)+ToTensor become PIL LANCZOS +
numpy (identical arithmetic), cv2.resize(bilinear) becomes PIL BILINEAR, cv2.imwrite becomes PIL save.
The reference quirk of thresholding the *logit* at 0.5 for the visualisation mask (predict_simple.py:77) is
kept.  `--no_cuda` is accepted for CLI compatibility but raises: this package has no CPU compute path.

Options beyond the reference, all off by default (without them nothing here behaves differently):
`--device_vis` draws the overlay on the GPU (csrc/visualise.hip), byte for byte what `InferenceManager.visualise` -- the host path, kept
as it is -- gives for the same prediction: Pillow's mode-"F" BILINEAR restated, not the reference's cv2.resize; the JPEG encoder stays
on the host unless `--device_jpeg` (needs --device_vis) is given too: then a group's overlays stay on the device, are encoded there
(csrc/jpeg.hip) and the .jpg files are written from the returned bytes -- the files Pillow writes, byte for byte.  `--batch_size N` predicts a folder N files at a time, in sorted order: one forward pass, one copy of the predictions and
(with --device_vis) one overlay call and one copy of the overlays per group; the photos of a group may differ in size, and the same
files are written under the same names.  `--device_decode` (needs --device_resize) reads the files' bytes and decodes the baseline
JPEGs among them on the GPU (csrc/jpeg_decode.hip), straight into the packed buffer the resize and the overlay share -- the bytes Pillow
decodes; every other file (PNG, progressive JPEG, ...) is decoded by Pillow and copied into the same buffer: the inference pipelines'
decode stage (datasets/decode_stage.py), used blockingly on one slot.  A batched forward pass
differs from per-image passes at fp32 round-off -- the small
convolutions split their K loop by a rule that depends on the batch size -- so a .npy of a batched run is within the contract's 1e-4 of
its channel maximum of the per-image one, not bit-equal; every overlay still equals `visualise` of its own .npy.
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

from .model_manager import ModelManager
from .utils import MODEL_DIR, model_folder, pil_loader, sigmoid_to_depth

class _LazyOriginals:
    """the photos of a group that were decoded into a device buffer: one is copied back only when the host path asks for it"""

    def __init__(self, packed, shapes):
        self.packed, self.shapes = packed, shapes

    def __getitem__(self, n):
        at = sum(h * w * 3 for h, w in self.shapes[:n])
        h, w = self.shapes[n]
        return Image.fromarray(self.packed[at:at + h * w * 3].cpu().numpy().reshape(h, w, 3))


MODEL_HEIGHT_WIDTH = {"kitti": (192, 640), "matterport": (512, 640), "handheld": (256, 448)}   # predict_simple.py:21-25
IMAGE_EXTENSIONS = {".jpg", ".jpeg", ".png"}


def preprocess(pil_image, height_width, device_resize=False):
    """Resize((H,W), ANTIALIAS) + ToTensor + [None] (predict_simple.py:51-60) -> float32 [1,3,H,W] in [0,1].
    device_resize=True: the decoded frame is uploaded once and both steps run on the GPU (csrc/reader.hip: Pillow's LANCZOS byte for
    byte, then the division by 255); the result is a device tensor bit-equal to the host path's."""
    h, w = height_width
    if device_resize:
        from . import ops
        return ops.load_images_u8([np.asarray(pil_image, dtype=np.uint8)], h, w)
    resized = pil_image.resize((w, h), Image.LANCZOS)
    arr = np.asarray(resized, dtype=np.uint8).astype(np.float32) / 255.0
    return torch.from_numpy(arr).permute(2, 0, 1)[None].contiguous()


class InferenceManager:
    def __init__(self, model_name, save_dir, use_cuda=True, save_visualisations=True, weights_path=None, model_manager=None,
                 device_resize=False, device_vis=False, batch_size=1, device_jpeg=False, device_decode=False):
        if not use_cuda or not torch.cuda.is_available():
            raise RuntimeError("footprints_amd.predict_simple needs a MI355X: the package has no CPU compute path "
                               "(--no_cuda is accepted for CLI compatibility only)")
        self.model_name = model_name
        self.height_width = MODEL_HEIGHT_WIDTH[model_name]
        if model_manager is None:
            model_manager = ModelManager(is_inference=True, use_cuda=True)
            model_manager.load_model(weights_path=weights_path or model_folder(model_name))
        self.model_manager = model_manager
        self.model_manager.model.eval()
        self.model_manager.model.inference_scales = ("1/1",)      # only the full-resolution prediction is consumed below
        self.device_resize = bool(device_resize)
        self.device_vis, self.batch_size = bool(device_vis), int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.device_jpeg = bool(device_jpeg)
        if self.device_jpeg and not self.device_vis:
            raise ValueError("device_jpeg encodes the overlays where device_vis draws them: it needs device_vis")
        self.device_decode = bool(device_decode)
        if self.device_decode and not self.device_resize:
            raise ValueError("device_decode decodes into the buffer device_resize reads: it needs device_resize")
        self._stage = self._slot = None                 # device_decode: the decode stage and its one slot, built at first use
        self.overlay_hook = None       # callable(file stem, uint8 [h, w, 3]): sees every overlay before it is encoded
        self.save_dir = save_dir
        os.makedirs(os.path.join(save_dir, "outputs"), exist_ok=True)
        self.save_visualisations = save_visualisations
        if save_visualisations:
            os.makedirs(os.path.join(save_dir, "visualisations"), exist_ok=True)

    def predict_array(self, pil_image):
        x = preprocess(pil_image, self.height_width, self.device_resize).cuda()
        with torch.no_grad():
            pred = self.model_manager.model(x)
        return pred["1/1"].cpu().numpy().squeeze(0)          # [4,H,W]

    def predict_for_single_image(self, image_path):
        if self.device_vis or self.device_decode:
            return self.predict_for_images([image_path])[0]
        print("Predicting for {}".format(image_path))
        original = pil_loader(image_path)
        pred = self.predict_array(original)
        filename, _ = os.path.splitext(os.path.basename(image_path))
        npy_save_path = os.path.join(self.save_dir, "outputs", filename + ".npy")
        print("└> Saving predictions to {}".format(npy_save_path))
        np.save(npy_save_path, pred)
        if self.save_visualisations:
            self._save_visualisation(filename, self.visualise(pred, original))
        return pred

    def _save_visualisation(self, filename, vis, encoded=None):
        """encoded: the file's bytes when the device has encoded the overlay already"""
        if self.overlay_hook is not None:
            self.overlay_hook(filename, vis)
        vis_save_path = os.path.join(self.save_dir, "visualisations", filename + ".jpg")
        print("└> Saving visualisation to {}".format(vis_save_path))
        if encoded is not None:
            with open(vis_save_path, "wb") as fh:
                fh.write(encoded)
            return
        Image.fromarray(vis).save(vis_save_path, quality=95)

    def predict_for_images(self, image_paths):
        """one group of files in ONE forward pass: the same artefacts as predict_for_single_image on each; returns [B,4,H,W].
        With device_resize the decoded photos are uploaded once, for the resize and for the overlay."""
        from . import ops
        for p in image_paths:
            print("Predicting for {}".format(p))
        h, w = self.height_width
        packed = None
        originals = None if self.device_decode else [pil_loader(p) for p in image_paths]
        if self.device_decode:
            d = self._decode_packed(image_paths)
            packed = d["src"][:d["total"]]
            originals = _LazyOriginals(packed, d["shapes"])
            x = ops.to_tensor_u8(ops.resize_u8_packed(packed, d["total"], d["records"], d["n"], h, w, 3, d["max_h"], d["max_w"], self._stage.tables))
        elif self.device_resize:
            arrays = [np.asarray(o, dtype=np.uint8) for o in originals]
            tables = ops.resize_table_set("cuda")
            host, records, total, cn, max_h, max_w = ops.resize_pack(arrays, h, w, tables)
            packed = torch.from_numpy(host).cuda()
            x = ops.to_tensor_u8(ops.resize_u8_packed(packed, total, torch.from_numpy(records).cuda(), len(arrays), h, w, cn, max_h, max_w, tables))
        else:
            x = torch.cat([preprocess(o, self.height_width) for o in originals]).cuda()
        with torch.no_grad():
            pred_dev = self.model_manager.model(x)["1/1"].contiguous()
        preds = pred_dev.cpu().numpy()                           # [B,4,H,W]: one copy for the group
        overlays, files = None, None
        if self.save_visualisations and self.device_vis:
            shapes = originals.shapes if self.device_decode else [(o.size[1], o.size[0]) for o in originals]
            source = dict(packed=packed, shapes=shapes) if packed is not None else dict(originals=[np.asarray(o, dtype=np.uint8) for o in originals])
            if self.device_jpeg:
                files, overlays = self._encode_overlays(*ops.vis_overlay_device(pred_dev, **source))
            else:
                overlays = ops.vis_overlay(pred_dev, **source)
        for i, path in enumerate(image_paths):
            filename, _ = os.path.splitext(os.path.basename(path))
            npy_save_path = os.path.join(self.save_dir, "outputs", filename + ".npy")
            print("└> Saving predictions to {}".format(npy_save_path))
            np.save(npy_save_path, preds[i])
            if files is not None:
                self._save_visualisation(filename, overlays[i] if overlays is not None else None, files[i])
            elif self.save_visualisations:
                self._save_visualisation(filename, overlays[i] if overlays is not None else self.visualise(preds[i], originals[i]))
        return preds

    def _decode_packed(self, image_paths):
        """the photos of a group, decoded into one device buffer, one after the other -> what DecodeStage.finish returns: baseline JPEGs
        on the device from the files' bytes, everything else -- and a JPEG the device did not take -- by Pillow.  The decode stage of the
        pipelines (datasets/decode_stage.py), on one slot the manager keeps, used blockingly"""
        from . import ops
        from .datasets.decode_stage import DecodeStage, read_sample
        if self._stage is None or len(image_paths) > self._stage.batch_size:
            device = torch.device("cuda", torch.cuda.current_device())
            self._stage = DecodeStage(max(len(image_paths), self.batch_size), *self.height_width, ops.resize_table_set(device), device)
            self._slot = self._stage.new_slot()
        self._stage.queue(self._slot, [read_sample(p, True) for p in image_paths])
        return self._stage.finish(self._slot)

    def _encode_overlays(self, buffer, total, shapes):
        """the overlays of a group, lying in a device buffer -> (their .jpg files' bytes, the raw overlays for the hook or None)"""
        from . import ops
        records, _, max_h, max_w = ops.jpeg_records(shapes)
        scans, table = ops.jpeg_encode_packed(buffer, total, torch.from_numpy(records).to(buffer.device), len(shapes), 95, max_h=max_h, max_w=max_w)
        table = table.cpu().numpy()                              # waits
        files = ops.jpeg_files(scans[:int(table[len(shapes)][0])].cpu().numpy().tobytes(), table, shapes, 95)
        # the hook sees the raw overlay: only then is it copied
        return files, (ops.split_pictures(buffer[:total].cpu().numpy(), shapes) if self.overlay_hook is not None else None)

    @staticmethod
    def visualise(pred, original):
        """predict_simple.py:75-92: mask = resized LOGIT > 0.5 (quirk), plasma colormap of the hidden depth."""
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        size = original.size
        resize = lambda a: np.asarray(Image.fromarray(a.astype(np.float32), mode="F").resize(size, Image.BILINEAR))
        hidden_ground = resize(pred[1]) > 0.5
        hidden_depth = resize(sigmoid_to_depth(pred[3]))
        rgb = np.array(original) / 255.0
        if hidden_ground.any():
            _max, _min = hidden_depth[hidden_ground].max(), hidden_depth[hidden_ground].min()
            hidden_depth = (hidden_depth - _min) / max(_max - _min, 1e-12)
        cmap = plt.get_cmap("plasma", 256)(np.clip(hidden_depth, 0, 1))[:, :, :3]
        m = hidden_ground[:, :, None]
        vis = rgb * (1 - m) + cmap * m
        return (vis * 255).astype(np.uint8)

    def _image_files(self, folder):
        """image files directly inside `folder` (same extension filter as predict_simple.py:21-25), in sorted order"""
        return [os.path.join(folder, name) for name in sorted(os.listdir(folder))
                if os.path.splitext(name)[1].lower() in IMAGE_EXTENSIONS]

    def predict(self, image_path):
        """--image may name one file or a folder of images (predict_simple.py:94-110); returns the number of images written"""
        if os.path.isdir(image_path):
            targets = self._image_files(image_path)
        elif os.path.isfile(image_path):
            targets = [image_path]
        else:
            raise FileNotFoundError("--image: no such file or folder: %r" % (image_path,))
        if self.batch_size > 1:
            for i in range(0, len(targets), self.batch_size):
                self.predict_for_images(targets[i:i + self.batch_size])
            return len(targets)
        for path in targets:
            self.predict_for_single_image(path)
        return len(targets)


def parse_args(argv=None):
    """the reference's flag names and defaults (predict_simple.py:113-131) -- they are the CLI contract -- plus --weights"""
    ap = argparse.ArgumentParser(prog="footprints_amd.predict_simple",
                                 description="Footprints prediction for one image or a folder of images on the HIP engine.")
    ap.add_argument("--image", required=True, type=str, help="image file, or a folder whose image files are all predicted")
    ap.add_argument("--model", type=str, choices=sorted(MODEL_HEIGHT_WIDTH), help="which released model: fixes the input resolution")
    ap.add_argument("--no_cuda", action="store_true", help="accepted for compatibility; raises (no CPU compute path here)")
    ap.add_argument("--no_save_vis", action="store_true", help="write only the .npy predictions, no .jpg overlays")
    ap.add_argument("--save_dir", type=str, default="predictions", help="output root (outputs/ and visualisations/ below it)")
    ap.add_argument("--weights", type=str, default=None,
                    help="folder holding model.pth (default: %s/<model>; this build cannot download)" % MODEL_DIR)
    ap.add_argument("--device_resize", action="store_true", help="resize the decoded image on the GPU (same bytes as PIL's LANCZOS)")
    ap.add_argument("--device_vis", action="store_true", help="draw the overlays on the GPU (same bytes as the host path before the JPEG encoder)")
    ap.add_argument("--batch_size", type=int, default=1, help="files of a folder per forward pass (sorted order; sizes may differ)")
    ap.add_argument("--device_jpeg", action="store_true", help="with --device_vis: encode the overlays on the GPU too (the same .jpg files)")
    ap.add_argument("--device_decode", action="store_true",
                    help="with --device_resize: decode baseline JPEG files on the GPU too (the same pixels; other files by Pillow)")
    args = ap.parse_args(argv)
    if args.device_decode and not args.device_resize:
        ap.error("--device_decode needs --device_resize: it decodes into the buffer the resize reads")
    if args.device_jpeg and not args.device_vis:
        ap.error("--device_jpeg needs --device_vis: it encodes the overlays where they are drawn")
    return args


def main(argv=None):
    args = parse_args(argv)
    manager = InferenceManager(model_name=args.model, use_cuda=torch.cuda.is_available() and not args.no_cuda,
                               save_visualisations=not args.no_save_vis, save_dir=args.save_dir, weights_path=args.weights,
                               device_resize=args.device_resize, device_vis=args.device_vis, batch_size=args.batch_size,
                               device_jpeg=args.device_jpeg, device_decode=args.device_decode)
    manager.predict(image_path=args.image)


if __name__ == "__main__":
    main()
