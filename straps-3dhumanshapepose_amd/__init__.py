"""MI355X-native STRAPS hot path: ResNet encoder -> IEF regressor -> rot6d -> SMPL forward.

Host side mirrors the reference's nn.Module surface (names, signatures, state-dict keys); all
arithmetic runs in hand-written HIP kernels for gfx950 behind the C ABI in include/straps_hip.h
(loaded with ctypes, see hipabi.py).  There is NO CPU fallback: calling a module without the HIP
library / a GPU raises.
"""
from . import config, hipabi  # noqa: F401
from .synthetic_smpl import synthetic_smpl_model, synthetic_mean_params, load_smpl_model  # noqa: F401
from .resnet import ResNet, BasicBlock, Bottleneck, resnet18, resnet50  # noqa: F401
from .ief_module import IEFModule  # noqa: F401
from .regressor import SingleInputRegressor  # noqa: F401
from .infer import InferenceRegressor, flat_inference_params  # noqa: F401
from .train_abi import CompositeTrainer, flat_training_params, flat_bn_state  # noqa: F401
from .smpl import SMPL, ModelOutput, pack_smpl_model  # noqa: F401
from .rigid_transform_utils import rot6d_to_rotmat, batch_rodrigues  # noqa: F401
from .multi_task_loss import HomoscedasticUncertaintyWeightedMultiTaskLoss  # noqa: F401
from .nmr_renderer import NMRRenderer, WeakPerspectiveSilhouetteRenderer, WeakPerspectiveMeshRenderer, vertex_face_table  # noqa: F401
from .metrics import EvalMetricsTracker  # noqa: F401
from .predict import Predictor, create_proxy_representation_batch, heatmap_patch  # noqa: F401
from .fit import KeypointFitter, SilhouetteFitter, SubjectFitter, ScanFitter, MeasurementFitter, distance_field, pack_fit_model  # noqa: F401
from .measure import BodyMeasurer, default_measurements, tape_measurements, posed_measurements  # noqa: F401
from .validation import ValStep, EpochHistory  # noqa: F401
from . import cam_utils, label_conversions, augmentation, metrics, checkpoint_utils, image_utils, device_rng, measure, validation  # noqa: F401
