"""gandtr_amd -- MI355X-native implementation of the gandtr inference hot path.

Drop-in surface (mirrors the reference's own modules):
  hubconf.py / gandtr_amd.hub.model      cyclegan, hedngan, gem_vgg16_*, gem_resnet101_*
  gandtr_amd.components.model.network    MODEL_LABELS / initialize_model
  gandtr_amd.components.model.layers     ATTENTIONS, POOLINGS (geometric-median pooling of the embedder, Weiszfeld's iteration on the device), EdgeFilter
  gandtr_amd.components.data.wrapper     WRAPPERS_LABELS / initialize_wrappers
  gandtr_amd.components.data.dataset     DATASET_LABELS / initialize_dataset_loader (the GAN scenarios' data blocks, decoded and cropped on the device)
  gandtr_amd.learning.network            NETWORKS / initialize_network / SingleNetwork / CirSequentialNetwork
  gandtr_amd.stages                      infer, whiten, learn_lw_whitening (stage ABI)
"Next" rows of SURVEY.md section 8f (device paths beside the hot path):
  gandtr_amd.clahe / ingest / retrieval / whiten_learn
  gandtr_amd.retrieval                   topk / expand_queries / augment_database / knn_graph: the k best per query without the score matrix, aQE, DBA
  gandtr_amd.mining                  an epoch's training tuples: diverse anchors + hard negatives (create_epoch_tuples)
  gandtr_amd.components.optim.criterion  CRITERIA / initialize_criterion: contrastive and triplet loss of tuples (forward only)
  gandtr_amd.learning.validation         the loss validation of the fine-tuning scenario on the mined tuples (SingleValidation with a data key)
Compute: gandtr_amd/csrc (HIP kernels for gfx950) behind the C ABI in include/gandtr_hip.h.
"""
__version__ = "0.1.0"
