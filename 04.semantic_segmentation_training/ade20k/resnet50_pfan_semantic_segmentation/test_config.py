"""Benchmark copy of reference 04.semantic_segmentation_training/ade20k/resnet50_pfan_semantic_segmentation/test_config.py
(:20-53): network, 151 classes, 512-pixel canvas, CELoss and the collater are the train config's (the reference repeats them
literally; here they are taken from train_config.py next to this file); ADE20K validation is replaced by the synthetic
segmentation set, batch 16 / 8 workers as the reference sets them (SAICV_SEG_* shorten a smoke run of
tools/test_semantic_segmentation_model.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_config import config as _train  # noqa: E402


class config:
    network, num_classes, input_image_size = _train.network, _train.num_classes, _train.input_image_size
    model = _train.model
    trained_model_path = _train.trained_model_path
    test_criterion = _train.test_criterion
    test_dataset, test_collater = _train.test_dataset, _train.test_collater
    seed = 0
    batch_size = int(os.environ.get('SAICV_SEG_BATCH', 16))
    num_workers = int(os.environ.get('SAICV_SEG_WORKERS', 8))
