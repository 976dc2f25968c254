"""Benchmark copy of reference 16.universal_segmentation_training/16.0.semantic_segmentation_training/ade20k/
dinov3_vit_large_patch16_universal_segmentation/train_config.py (:21-104): network, 512-pixel canvas, 100 queries, 151 classes
(background included), UniversalSegmentationLoss with costs / weights 5, 5, 2 and no-object weight 0.1, global batch 128,
('Muon', lr 4e-4, weight decay 1e-3), CosineLR with one warm-up epoch over 100 epochs, AMP, as the reference sets them; the ADE20K
dataset + OpenCV resize is replaced by a synthetic label-map dataset at its final size and no pretrained backbone is loaded
(neither exists in the bench image).  SAICV_UNIVSEG_* shorten a smoke run of the entry script."""
import os
import sys

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
sys.path.append(BASE_DIR)

from SimpleAICV.universal_segmentation import models
from SimpleAICV.universal_segmentation import segmentation_losses
from SimpleAICV.universal_segmentation.datasets.syntheticdataset import SyntheticUniversalSegmentationDataset
from SimpleAICV.universal_segmentation.semantic_segmentation_common import (Normalize, RandomHorizontalFlip,
                                                                           SemanticSegmentationTrainCollater, load_state_dict)


class _Compose:

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, sample):
        for t in self.transforms:
            sample = t(sample)
        return sample


class config:
    network = os.environ.get('SAICV_UNIVSEG_MODEL', 'dinov3_vit_large_patch16_universal_segmentation')
    input_image_size = int(os.environ.get('SAICV_UNIVSEG_SIZE', 512))
    query_num = int(os.environ.get('SAICV_UNIVSEG_QUERIES', 100))
    # num_classes has background class
    num_classes = 151

    backbone_pretrained_path = ''
    model = models.__dict__[network](**{
        'backbone_pretrained_path': backbone_pretrained_path,
        'image_size': input_image_size,
        'query_num': query_num,
        'num_classes': num_classes,
    })

    trained_model_path = ''
    load_state_dict(trained_model_path, model)

    train_criterion = segmentation_losses.__dict__['UniversalSegmentationLoss'](**{
        'mask_cost': 5.0,
        'dice_cost': 5.0,
        'class_cost': 2.0,
        'num_classes': num_classes,
        'mask_loss_weight': 5.0,
        'dice_loss_weight': 5.0,
        'class_loss_weight': 2.0,
        'no_object_class_weight': 0.1,
    })

    # size of ADE20K training
    train_dataset = SyntheticUniversalSegmentationDataset(int(os.environ.get('SAICV_UNIVSEG_TRAIN', 20210)), input_image_size,
                                                          num_classes=num_classes, seed=0,
                                                          transform=_Compose([RandomHorizontalFlip(prob=0.5), Normalize()]))
    train_collater = SemanticSegmentationTrainCollater(resize=input_image_size)

    seed = 0
    # batch_size is total size
    batch_size = int(os.environ.get('SAICV_UNIVSEG_BATCH', 128))
    # num_workers is total workers
    num_workers = int(os.environ.get('SAICV_UNIVSEG_WORKERS', 32))
    accumulation_steps = 1

    optimizer = ('Muon', {'lr': 4e-4, 'weight_decay': 1e-3, 'exclude_muon_layer_name_list': []})
    scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})

    epochs = int(os.environ.get('SAICV_UNIVSEG_EPOCHS', 100))
    print_interval = int(os.environ.get('SAICV_UNIVSEG_PRINT', 10))
    save_interval = 20

    sync_bn = False
    use_amp = True
    use_compile = False
    compile_params = {'mode': 'default'}

    use_ema_model = False
    ema_model_decay = 0.9999
