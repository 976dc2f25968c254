"""Benchmark copy of reference 11.face_parsing_training/CelebAMask-HQ/resnet50_pfan_face_parsing/test_config.py (:20-66):
network, 19 classes, 512-pixel canvas, CELoss, the validation sets and the collater are the train config's (the reference repeats
them literally; here they are taken from train_config.py next to this file); batch 64 / 8 workers as the reference sets them
(SAICV_FP_* shorten a smoke run of tools/test_face_parsing_model.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_config import config as _train  # noqa: E402


class config:
    network, num_classes, input_image_size = _train.network, _train.num_classes, _train.input_image_size
    model = _train.model
    trained_model_path = _train.trained_model_path
    test_criterion = _train.test_criterion
    val_dataset_name_list, val_dataset_list, val_collater = _train.val_dataset_name_list, _train.val_dataset_list, _train.val_collater
    seed = 0
    batch_size = int(os.environ.get('SAICV_FP_BATCH', 64))
    num_workers = int(os.environ.get('SAICV_FP_WORKERS', 8))
