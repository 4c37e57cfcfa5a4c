"""Entry point -- counterpart of footprints/main.py:8-26: `python -m footprints_amd.main --mode train ...`.

`--mode train` trains from the folders the config file names, like the reference: `--config_path`'s [training_dataset]['dataset' |
'training_data'] and splits/<dataset>/{train,val}.txt relative to the working directory (datasets/training.py: the file readers on a pool
of threads; the frame's resize, the label maps' cv2 resizes, the depth-mask filter, flip, jitter and label algebra on the device).  With
`--synthetic_steps N` it runs over the synthetic loader the benchmark uses instead, and no file is read.  Training writes TensorBoard
files under <log_path>/<model_name>/{train,val} every `--log_freq` steps (training/logger.py) unless `--no_summaries` is given.  `--mode inference` is the
reference's test-set program (footprints/evaluation/inference.py:31-96): the test split of `--inference_data_type` through the network, one
.npy (and with --save_test_visualisations one .jpg) per frame -- the input of `evaluation/evaluate_model.py --predictions`."""
from .options import Options
from .parallel import DistContext
from .training.train import SyntheticLoader, TrainManager


def run_inference(opt, model_manager=None):
    """the reference's InferenceManager.__init__ + create_dataloaders + run (evaluation/inference.py:36-96): the config file's
    [inference_data_type]['dataset'], splits/<type>/test.txt relative to the working directory, and the save path --inference_save_path
    or <load_path>/<type>_predictions"""
    import os
    import yaml
    from .datasets.inference import get_inference_dataset_class
    from .evaluation.inference import InferenceManager
    print("In inference mode!")
    with open(opt.config_path) as fh:
        raw_data_path = yaml.safe_load(fh)[opt.inference_data_type]["dataset"]
    with open(os.path.join("splits", opt.inference_data_type, "test.txt")) as fh:
        test_files = fh.read().splitlines()
    save_path = opt.inference_save_path
    if save_path is None:
        save_path = os.path.join(opt.load_path, "{}_predictions".format(opt.inference_data_type))
    print("saving output to {}".format(save_path))
    dataset = get_inference_dataset_class(opt.inference_data_type)(raw_data_path, test_files, opt.height, opt.width)
    manager = InferenceManager(load_path=opt.load_path, model_manager=model_manager, save_path=save_path,
                               save_test_visualisations=opt.save_test_visualisations, device_jpeg=getattr(opt, "device_jpeg", False))
    print("running inference...")
    counters = manager.run_dataset(dataset, opt.batch_size, num_workers=opt.num_workers, device_decode=getattr(opt, "device_decode", False))
    print("finished testing!")
    return manager, counters


def main(argv=None, model_manager=None):
    opt = Options().parse(argv)
    if opt.mode == "train":
        # FIRST thing under a launcher: select this rank's GPU (LOCAL_RANK) and join the host group before ANY loader, assembler,
        # pinned buffer or stream exists -- a DeviceBatchAssembler built earlier would put its slots and its copy stream on GPU 0 on every rank
        ctx = DistContext.from_env()
        if ctx.is_main:
            print("In training mode!")
        summaries = not getattr(opt, "no_summaries", False)      # train.py:47-50: the reference always writes them
        if opt.synthetic_steps <= 0:
            # the reference's create_dataloaders over the device path; under a data-parallel launch TrainManager shards the train source
            from .datasets.training import create_dataloaders
            train, val = create_dataloaders(opt, device_decode=getattr(opt, "device_decode", False))
            return TrainManager(opt, train_loader=train, val_loader=val, dist_context=ctx, summaries=summaries).train()
        if opt.device_augment and opt.training_dataset == "kitti":
            # row N3: host samples as the file readers deliver them -> pinned double-buffered H2D -> flip / jitter / label kernels
            from .datasets import DeviceBatchAssembler, DeviceLoader, SyntheticSampleSource
            asm = DeviceBatchAssembler(opt.batch_size, opt.height, opt.width, dataset="kitti", no_depth_mask=opt.no_depth_mask,
                                       project_down_baseline=opt.project_down_baseline, moving_objects_method=opt.moving_objects_method)
            train = DeviceLoader(SyntheticSampleSource(opt.batch_size, opt.height, opt.width, opt.synthetic_steps), asm, is_train=True)
        else:
            train = SyntheticLoader(opt.batch_size, opt.height, opt.width, opt.synthetic_steps)
        val = SyntheticLoader(opt.batch_size, opt.height, opt.width, max(1, opt.val_batches), seed=11)
        # under torch.distributed.run (WORLD_SIZE > 1) TrainManager turns into one replica of a data-parallel run: --batch_size is the
        # per-GPU batch, --synthetic_steps the number of GLOBAL batches per epoch (each rank trains on every world-th one)
        TrainManager(opt, train_loader=train, val_loader=val, dist_context=ctx, summaries=summaries).train()
    elif opt.mode == "inference":
        return run_inference(opt, model_manager)[1]
    else:
        raise NotImplementedError


if __name__ == "__main__":
    main()
