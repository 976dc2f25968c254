"""Benchmark copy of reference 04.semantic_segmentation_training/ade20k/resnet50_pfan_semantic_segmentation/train_config.py
(:20-117): network, 151 classes (background included), 512-pixel canvas, CELoss with ratio 1.0, global batch 32, AdamW 1e-4,
CosineLR with one warm-up epoch over 100 epochs, AMP, as the reference sets them; the ADE20K dataset + OpenCV transform block is
replaced by a synthetic segmentation dataset and no pretrained backbone is loaded (neither exists in the bench image)."""
import os
import sys

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.append(BASE_DIR)

from SimpleAICV.semantic_segmentation import models
from SimpleAICV.semantic_segmentation import losses
from SimpleAICV.semantic_segmentation.datasets.syntheticdataset import SyntheticSemanticSegmentationDataset
from SimpleAICV.semantic_segmentation.common import SemanticSegmentationCollater, load_state_dict


class config:
    network = 'resnet50_pfan_semantic_segmentation'
    input_image_size = 512
    # num_classes has background class
    num_classes = 151

    backbone_pretrained_path = ''
    model = models.__dict__[network](**{'backbone_pretrained_path': backbone_pretrained_path, 'num_classes': num_classes})

    trained_model_path = ''
    load_state_dict(trained_model_path, model)

    loss_list = ['CELoss']
    loss_ratio = {'CELoss': 1.0}
    train_criterion = {loss_name: losses.__dict__[loss_name](**{}) for loss_name in loss_list}
    test_criterion = losses.__dict__['CELoss'](**{})

    # sizes of ADE20K training / validation; SAICV_SEG_* shorten a smoke run of the entry script
    train_dataset = SyntheticSemanticSegmentationDataset(int(os.environ.get('SAICV_SEG_TRAIN', 20210)), 384, 512,
                                                         num_classes=num_classes, seed=0)
    test_dataset = SyntheticSemanticSegmentationDataset(int(os.environ.get('SAICV_SEG_TEST', 2000)), 384, 512,
                                                        num_classes=num_classes, seed=1)
    train_collater = SemanticSegmentationCollater(resize=input_image_size)
    test_collater = SemanticSegmentationCollater(resize=input_image_size)

    seed = 0
    # batch_size is total size
    batch_size = int(os.environ.get('SAICV_SEG_BATCH', 32))
    # num_workers is total workers
    num_workers = int(os.environ.get('SAICV_SEG_WORKERS', 32))
    accumulation_steps = 1

    optimizer = ('AdamW', {'lr': 1e-4, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})

    epochs = int(os.environ.get('SAICV_SEG_EPOCHS', 100))
    eval_epoch = [1] + [i for i in range(epochs) if i % 10 == 0]
    print_interval = int(os.environ.get('SAICV_SEG_PRINT', 100))

    save_model_metric = 'mean_iou'

    sync_bn = False
    use_amp = True
    use_compile = False
    compile_params = {'mode': 'default'}

    use_ema_model = False
    ema_model_decay = 0.9999
