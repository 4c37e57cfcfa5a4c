"""Command-line options of the ground-segmentation trainer: the reference's flags and defaults
(footprints/preprocessing/segmentation/options.py)."""
import argparse


class SegmentationOptions:

    def __init__(self):
        self.options = None
        p = self.parser = argparse.ArgumentParser()
        # universal
        p.add_argument("--mode", help="training or testing mode", type=str, choices=["train", "inference"], default="train")
        p.add_argument("--config_path", default="paths.yaml", help="path to config file containing path information", type=str)
        p.add_argument("--height", help="height of input images", type=int, default=192)
        p.add_argument("--width", help="width of input images", type=int, default=640)
        p.add_argument("--no_PSP", action="store_true")
        # training
        p.add_argument("--training_datasets", help="dataset(s) to train on", type=str, nargs="+", choices=["ADE20K", "cityscapes", "matterport"],
                       default=["ADE20K", "cityscapes"])
        p.add_argument("--epochs", help="number of epochs to train for", type=int, default=20)
        p.add_argument("--log_freq", help="sets the frequency of logs", type=int, default=250)
        p.add_argument("--batch_size", help="number of images in each batch", type=int, default=12)
        p.add_argument("--val_batches", help="number of validation batches to average over", type=int, default=10)
        p.add_argument("--lr", help="the learning rate", type=float, default=1e-4)
        p.add_argument("--num_workers", type=int, default=4,
                       help="the number of threads that read the files of upcoming batches (validation: at most 2); 0: one batch at a time "
                            "on the staging thread")
        p.add_argument("--model_name", help="the name of the model for saving", type=str, default="model")
        p.add_argument("--log_path", help="the path to save logs and trained models to", type=str, default="./logs")
        p.add_argument("--no_summaries", action="store_true",
                       help="train without writing TensorBoard files under <log_path>/<model_name>/{train,val}")
        # testing
        p.add_argument("--load_path", help="the model path to load from", type=str)
        p.add_argument("--test_save_folder", help="folder to save results to - added to training_data path from config", type=str,
                       default="ground_seg")
        p.add_argument("--test_data_type", choices=["kitti", "matterport"], default="kitti")
        p.add_argument("--save_test_visualisations", action="store_true")
        p.add_argument("--device_jpeg", action="store_true",
                       help="with --save_test_visualisations: encode the pictures on the GPU (same files as Pillow writes)")
        p.add_argument("--device_decode", action="store_true",
                       help="decode baseline JPEG frames on the GPU; what the decoder does not take (PNG, progressive files, ...) goes to "
                            "Pillow, and the results are the same either way.  Inference mode: one batch ahead of the network.  Training "
                            "mode: inside batch assembly, only the rectangle of a frame that its crop window needs")

    def parse(self, args=None):
        self.options = self.parser.parse_args(args)
        return self.options
