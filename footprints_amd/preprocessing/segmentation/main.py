"""python -m footprints_amd.preprocessing.segmentation.main: train the ground-segmentation network on device-assembled batches (TensorBoard
files under <log_path>/<model_name>/{train,val} every `--log_freq` steps unless `--no_summaries` is given; the files of upcoming batches
read on `--num_workers` threads, and with `--device_decode` the baseline JPEGs among them decoded on the device), or
(`--mode inference`) run the trained network over a dataset's train and val frames and write the ground-probability maps that
ground_truth_generation reads (reference: footprints/preprocessing/segmentation/main.py)."""
from .options import SegmentationOptions


def main(args=None):
    options = SegmentationOptions().parse(args)
    if options.mode == "train":
        print("In training mode!")
        from .train import Trainer
        Trainer(options, summaries=not options.no_summaries).train()      # train.py:58-62: the reference always writes them
    elif options.mode == "inference":
        print("In inference mode!")
        from .inference import Tester
        Tester(options).test()
    else:
        raise NotImplementedError


if __name__ == "__main__":
    main()
