"""python -m footprints_amd.preprocessing.segmentation.main: train the ground-segmentation network on device-assembled batches
(reference: footprints/preprocessing/segmentation/main.py; its inference mode is segmentation/inference.py's InferenceManager)."""
from .options import SegmentationOptions


def main(args=None):
    options = SegmentationOptions().parse(args)
    if options.mode != "train":
        raise NotImplementedError("inference runs through footprints_amd.preprocessing.segmentation.inference.InferenceManager")
    print("In training mode!")
    from .train import Trainer
    Trainer(options).train()


if __name__ == "__main__":
    main()
