"""python -m footprints_amd.preprocessing.segmentation.main: train the ground-segmentation network on device-assembled batches, or
(`--mode inference`) run the trained network over a dataset's train and val frames and write the ground-probability maps that
ground_truth_generation reads (reference: footprints/preprocessing/segmentation/main.py)."""
from .options import SegmentationOptions


def main(args=None):
    options = SegmentationOptions().parse(args)
    if options.mode == "train":
        print("In training mode!")
        from .train import Trainer
        Trainer(options).train()
    elif options.mode == "inference":
        print("In inference mode!")
        from .inference import Tester
        Tester(options).test()
    else:
        raise NotImplementedError


if __name__ == "__main__":
    main()
