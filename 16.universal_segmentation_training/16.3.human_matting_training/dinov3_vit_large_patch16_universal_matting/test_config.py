"""Benchmark copy of reference 16.universal_segmentation_training/16.3.human_matting_training/
dinov3_vit_large_patch16_universal_matting/test_config.py (:20-72): network, canvas, queries and classes are the train config's next
to this file; UniversalMattingDecoder(topk 1, score 0.1), batch 8 / 8 workers, thresh [0.2], squared_beta 0.3 as the reference sets
them; the P3M validation sets are replaced by one synthetic matte set and no trained weights are loaded (SAICV_UNIMAT_* shorten a
smoke run of tools/test_universal_segmentation_model_for_human_matting_dataset.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_config import config as _train, _Compose  # noqa: E402

from SimpleAICV.universal_segmentation import matting_decode  # noqa: E402
from SimpleAICV.universal_segmentation.datasets.syntheticmattingdataset import SyntheticUniversalMattingDataset  # noqa: E402
from SimpleAICV.universal_segmentation.human_matting_common import HumanMattingTestCollater, Normalize  # noqa: E402


class config:
    network, num_classes, input_image_size, query_num = _train.network, _train.num_classes, _train.input_image_size, _train.query_num
    model = _train.model
    trained_model_path = _train.trained_model_path
    decoder = matting_decode.__dict__['UniversalMattingDecoder'](**{
        'topk': 1,
        'min_score_threshold': 0.1,
    })
    # the complete validation set comes first
    val_dataset_name_list = [['synthetic_mattes']]
    val_dataset_list = [SyntheticUniversalMattingDataset(int(os.environ.get('SAICV_UNIMAT_TEST', 1000)), input_image_size[0], seed=1,
                                                         transform=_Compose([Normalize()]))]
    val_collater = HumanMattingTestCollater(resize=input_image_size[0])
    seed = 0
    batch_size = int(os.environ.get('SAICV_UNIMAT_BATCH', 8))
    num_workers = int(os.environ.get('SAICV_UNIMAT_WORKERS', 8))

    thresh = [0.2]
    squared_beta = 0.3
