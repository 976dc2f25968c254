"""Benchmark copy of reference 09.ocr_text_recognition_training/resnet50_ctc_model/test_config.py: network, converter, character
table, CTCLoss, the validation sets and the collater are the train config's (the reference repeats them literally; here they are
taken from train_config.py next to this file); batch 256 / 8 workers as the reference sets them (SAICV_OCR_* shorten a smoke run of
tools/test_text_recognition_model.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_config import config as _train  # noqa: E402


class config:
    network, resize_h, str_max_length = _train.network, _train.resize_h, _train.str_max_length
    all_char_table, converter, num_classes = _train.all_char_table, _train.converter, _train.num_classes
    model = _train.model
    trained_model_path = _train.trained_model_path
    test_criterion = _train.test_criterion
    val_dataset_name_list, val_dataset_list, test_collater = _train.val_dataset_name_list, _train.val_dataset_list, _train.test_collater
    seed = 0
    batch_size = int(os.environ.get('SAICV_OCR_BATCH', 256))
    num_workers = int(os.environ.get('SAICV_OCR_WORKERS', 8))
