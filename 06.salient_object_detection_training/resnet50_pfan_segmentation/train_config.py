"""Benchmark copy of reference 06.salient_object_detection_training/resnet50_pfan_segmentation/train_config.py (:19-141): network,
1024 x 1024 canvas, BCELoss + BCEIouloss at ratio 1.0, global batch 64, AdamW 1e-4, CosineLR with one warm-up epoch over 100
epochs, thresh [0.2], squared_beta 0.3, checkpoints by miou_average, AMP, as the reference sets them; the salient-object dataset +
OpenCV transform block is replaced by a synthetic dataset of soft masks and no pretrained backbone is loaded (neither exists in the
bench image)."""
import os
import sys

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(BASE_DIR)

from SimpleAICV.salient_object_detection import models
from SimpleAICV.salient_object_detection import losses
from SimpleAICV.salient_object_detection.datasets.syntheticdataset import SyntheticSalientObjectDetectionDataset
from SimpleAICV.salient_object_detection.common import SalientObjectDetectionSegmentationCollater, load_state_dict


class config:
    # SAICV_SAL_* shorten a smoke run of the entry scripts
    input_image_size = [int(os.environ.get('SAICV_SAL_SIZE', 1024))] * 2
    network = 'resnet50_pfan_segmentation'

    backbone_pretrained_path = ''
    model = models.__dict__[network](**{'backbone_pretrained_path': backbone_pretrained_path})

    trained_model_path = ''
    load_state_dict(trained_model_path, model)

    loss_list = ['BCELoss', 'BCEIouloss']
    loss_ratio = {'BCELoss': 1.0, 'BCEIouloss': 1.0}
    train_criterion = {loss_name: losses.__dict__[loss_name]() for loss_name in loss_list}
    test_criterion = losses.__dict__['BCELoss']()

    train_dataset = SyntheticSalientObjectDetectionDataset(int(os.environ.get('SAICV_SAL_TRAIN', 30000)), input_image_size[0],
                                                           input_image_size[1], seed=0)
    # the complete validation set is the first entry of the list: the entry script checkpoints by its result
    val_dataset_name_list = [['AM2K', 'DIS5K', 'HRS10K', 'HRSOD', 'UHRSD']]
    val_dataset_list = []
    for per_sub_dataset_list in val_dataset_name_list:
        val_dataset_list.append(SyntheticSalientObjectDetectionDataset(int(os.environ.get('SAICV_SAL_TEST', 2000)), input_image_size[0],
                                                                       input_image_size[1], seed=1 + len(val_dataset_list)))
    train_collater = SalientObjectDetectionSegmentationCollater(resize=input_image_size[0])
    val_collater = SalientObjectDetectionSegmentationCollater(resize=input_image_size[0])

    seed = 0
    # batch_size is total size
    batch_size = int(os.environ.get('SAICV_SAL_BATCH', 64))
    # num_workers is total workers
    num_workers = int(os.environ.get('SAICV_SAL_WORKERS', 32))
    accumulation_steps = 1

    optimizer = ('AdamW', {'lr': 1e-4, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})

    epochs = int(os.environ.get('SAICV_SAL_EPOCHS', 100))
    eval_epoch = [1] + [i for i in range(epochs) if i % 10 == 0]
    print_interval = int(os.environ.get('SAICV_SAL_PRINT', 100))
    save_interval = 10

    save_model_metric = 'miou_average'
    thresh = [0.2]
    squared_beta = 0.3

    sync_bn = False
    use_amp = True
    use_compile = False
    compile_params = {'mode': 'default'}
    use_step_graph = os.environ.get('SAICV_SAL_GRAPH', '0') == '1'

    use_ema_model = False
    ema_model_decay = 0.9999
