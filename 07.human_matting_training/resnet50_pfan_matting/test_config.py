"""Benchmark copy of reference 07.human_matting_training/resnet50_pfan_matting/test_config.py (:19-62): network, 1024 x 1024 canvas,
GlobalTrimapCELoss, thresh [0.2], squared_beta 0.3 and the collater are the train config's (the reference repeats them literally;
here they are taken from train_config.py next to this file); the validation sets are the synthetic ones, batch 16 / 8 workers as
the reference sets them (SAICV_MAT_* shorten a smoke run of tools/test_human_matting_model.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_config import config as _train  # noqa: E402


class config:
    network, input_image_size = _train.network, _train.input_image_size
    model = _train.model
    trained_model_path = _train.trained_model_path
    test_criterion = _train.test_criterion
    val_dataset_name_list, val_dataset_list, val_collater = _train.val_dataset_name_list, _train.val_dataset_list, _train.val_collater
    seed = 0
    batch_size = int(os.environ.get('SAICV_MAT_BATCH', 16))
    num_workers = int(os.environ.get('SAICV_MAT_WORKERS', 8))
    thresh, squared_beta = _train.thresh, _train.squared_beta
