"""Training-label generation on the device (reference footprints/preprocessing/ground_truth_generation/): hidden ground depths,
moving-object masks and depth masks, from dataset folders (data_loader.py, `main`) or from any loader object handed to a generator."""
from .data_loader import FrameCache, KITTILoader, MatterportLoader  # noqa: F401
from .geometry import BatchProjector, fit_plane  # noqa: F401
from .ground_truth_generator import (GroundTruthGenerator, KITTIDepthMaskingGenerator, KITTIGroundTruthGenerator,  # noqa: F401
                                     KITTIMovingObjectDetector, MatterportDepthMaskingGenerator, MatterportGroundTruthGenerator,
                                     generator_class, get_options, main)
