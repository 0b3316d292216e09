"""qsparse_amd -- MI355X-native quantize/prune operators with the API of mlzxy/qsparse v2.0.1.

Drop-in for the reference's training hot path: ``quantize()``, ``prune()``, ``convert()`` and the layers,
callbacks and helpers they expose (reference qsparse/__init__.py:2-8).  GPU tensors are processed by
hand-written HIP kernels for gfx950 behind a C ABI (``include/qsparse_hip.h``,
``qsparse_amd/libqsparse_hip.so``); see DESIGN.md.
"""
from qsparse_amd.batch import WeightBatcher
from qsparse_amd.convert import convert
from qsparse_amd.export import LayerExport, QuantizedTensor, export_integer
from qsparse_amd.fuse import fuse_bn
from qsparse_amd.graphs import resync_host_state
from qsparse_amd.mx_bmm import MXMultiheadAttention, mx_attention, mx_bmm
from qsparse_amd.mx_batched_train import MXTrainMultiheadAttention, mx_attention_train, mx_bmm_train, mx_quantize_2way_batched
from qsparse_amd.mx_conv import MXConv2d, mx_conv2d
from qsparse_amd.mx_conv_train import MXTrainConv2d, mx_conv2d_train, mx_conv2d_weight_grad
from qsparse_amd.mx_conv_transpose import MXConvTranspose2d, mx_conv2d_input_grad, mx_conv_transpose2d
from qsparse_amd.mx_gemm import MXActivation, MXLinear, MXTrainLinear, mx_linear, mx_matmul, mx_quantize_2way
from qsparse_amd.mx_glu import (MXGatedMoEFeedForward, MXGLULinear, MXGroupedGLULinear, mx_glu_deinterleave, mx_glu_interleave,
                                mx_glu_matmul, mx_grouped_glu_matmul)
from qsparse_amd.mx_glu_train import (MXTrainGatedMoEFeedForward, MXTrainGLULinear, MXTrainGroupedGLULinear, mx_glu_backward_quantize,
                                      mx_glu_linear, mx_grouped_glu_linear)
from qsparse_amd.mx_grouped import MXGroupedLinear, MXMoEFeedForward, mx_grouped_matmul
from qsparse_amd.mx_grouped_train import MXTrainGroupedLinear, MXTrainMoEFeedForward, mx_grouped_linear, mx_grouped_weight_grad
from qsparse_amd.mx_norm import (MXAddNormLinear, MXLayerNorm, MXRMSNorm, MXTrainAddNormLinear, MXTrainNormLinear, mx_add_norm_linear,
                                 mx_add_norm_quantize, mx_norm_backward, mx_norm_linear, mx_norm_quantize)
from qsparse_amd.mx_rope import mx_rope, mx_rope_quantize, mx_rope_table
from qsparse_amd.mx_softmax import mx_softmax_backward_quantize, mx_softmax_quantize
from qsparse_amd.quantize import (AdaptiveQuantizer, DecimalQuantizer, MXQuantizer, ScalerQuantizer, quantize,
                                  quantize_with_decimal, quantize_with_line, quantize_with_mx, quantize_with_scaler)
from qsparse_amd.sparse import (MagnitudePruningCallback, UniformPruningCallback, devise_layerwise_pruning_schedule,
                                prune)
from qsparse_amd.util import (auto_name_prune_quantize_layers, calculate_mask_given_importance, extra_state_dict,
                              load_extra_state_dict, preload_qsparse_state_dict)
from qsparse_amd.util import get_option as get_qsparse_option
from qsparse_amd.util import set_options as set_qsparse_options

from qsparse_amd.util import PINNED_TORCH, check_torch_pin

__version__ = "2.0.1+mi355x.1"
check_torch_pin()      # warns once under a torch other than the one the staged means' summation order was taken from
