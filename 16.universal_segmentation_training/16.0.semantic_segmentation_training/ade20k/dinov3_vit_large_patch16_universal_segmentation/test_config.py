"""Benchmark copy of reference 16.universal_segmentation_training/16.0.semantic_segmentation_training/ade20k/
dinov3_vit_large_patch16_universal_segmentation/test_config.py (:21-66): network, canvas, queries and classes are the train
config's next to this file; UniversalSegmentationDecoder(topk 100, score 0.1, mask 0.5, binary), batch 16 / 8 workers as the
reference sets them; ADE20K validation is replaced by the synthetic label-map set and no trained weights are loaded
(SAICV_UNIVSEG_* shorten a smoke run of tools/test_universal_segmentation_model_for_semantic_segmentation_dataset.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_config import config as _train, _Compose  # noqa: E402

from SimpleAICV.universal_segmentation import segmentation_decode  # noqa: E402
from SimpleAICV.universal_segmentation.datasets.syntheticdataset import SyntheticUniversalSegmentationDataset  # noqa: E402
from SimpleAICV.universal_segmentation.semantic_segmentation_common import Normalize, SemanticSegmentationTestCollater  # noqa: E402


class config:
    network, num_classes, input_image_size, query_num = _train.network, _train.num_classes, _train.input_image_size, _train.query_num
    model = _train.model
    decoder = segmentation_decode.__dict__['UniversalSegmentationDecoder'](**{
        'topk': 100,
        'min_score_threshold': 0.1,
        'mask_threshold': 0.5,
        'binary_mask': True,
    })
    trained_model_path = _train.trained_model_path
    # size of ADE20K validation
    test_dataset = SyntheticUniversalSegmentationDataset(int(os.environ.get('SAICV_UNIVSEG_TEST', 2000)), input_image_size,
                                                         num_classes=num_classes, seed=1, transform=_Compose([Normalize()]))
    test_collater = SemanticSegmentationTestCollater(resize=input_image_size)
    seed = 0
    batch_size = int(os.environ.get('SAICV_UNIVSEG_BATCH', 16))
    num_workers = int(os.environ.get('SAICV_UNIVSEG_WORKERS', 8))
