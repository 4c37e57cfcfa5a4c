"""Training-label generation on the device (reference footprints/preprocessing/ground_truth_generation/): hidden ground depths,
moving-object masks and depth masks from loaded frames.  The file readers are not part of it: the generators take a loader object."""
from .geometry import BatchProjector, fit_plane  # noqa: F401
from .ground_truth_generator import (GroundTruthGenerator, KITTIDepthMaskingGenerator, KITTIGroundTruthGenerator,  # noqa: F401
                                     KITTIMovingObjectDetector, MatterportDepthMaskingGenerator, MatterportGroundTruthGenerator,
                                     get_options)
