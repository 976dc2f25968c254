"""Benchmark copy of reference 12.human_parsing_training/LIP/resnet50_pfan_human_parsing/train_config.py (:20-135):
network, 20 classes (background included), 512-pixel canvas, CELoss + IoULoss('softmax') with ratio 1.0 each, global batch 192,
AdamW 1e-4, CosineLR with one warm-up epoch over 100 epochs, evaluation at the last epoch, AMP, as the reference sets them; the
LIP dataset + OpenCV transform block is replaced by a synthetic parsing dataset and neither a pretrained backbone nor a trained
model is loaded (none exists in the bench image)."""
import os
import sys

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.append(BASE_DIR)

from SimpleAICV.human_parsing import models
from SimpleAICV.human_parsing import losses
from SimpleAICV.human_parsing.datasets.syntheticdataset import SyntheticHumanParsingDataset
from SimpleAICV.human_parsing.common import HumanParsingCollater, load_state_dict


class config:
    network = 'resnet50_pfan_human_parsing'
    # num_classes has background class
    num_classes = 20
    input_image_size = [512, 512]

    backbone_pretrained_path = ''
    model = models.__dict__[network](**{'backbone_pretrained_path': backbone_pretrained_path, 'num_classes': num_classes})

    trained_model_path = ''
    load_state_dict(trained_model_path, model)

    loss_list = ['CELoss', 'IoULoss']
    loss_ratio = {'CELoss': 1.0, 'IoULoss': 1.0}
    train_criterion = {}
    for loss_name in loss_list:
        if loss_name == 'IoULoss':
            train_criterion[loss_name] = losses.__dict__[loss_name](**{'logit_type': 'softmax'})
        else:
            train_criterion[loss_name] = losses.__dict__[loss_name](**{})
    test_criterion = losses.__dict__['CELoss'](**{})

    # sizes of LIP training / validation; SAICV_HP_* shorten a smoke run of the entry script
    train_dataset = SyntheticHumanParsingDataset(int(os.environ.get('SAICV_HP_TRAIN', 30462)), 512, 384, num_classes=num_classes,
                                                 seed=0)
    val_dataset_name_list = [['LIP']]
    val_dataset_list = []
    for i, per_sub_dataset_list in enumerate(val_dataset_name_list):
        val_dataset_list.append(SyntheticHumanParsingDataset(int(os.environ.get('SAICV_HP_TEST', 10000)), 512, 384, num_classes=num_classes,
                                                             seed=1 + i))
    train_collater = HumanParsingCollater(resize=input_image_size[0])
    val_collater = HumanParsingCollater(resize=input_image_size[0])

    seed = 0
    # batch_size is total size
    batch_size = int(os.environ.get('SAICV_HP_BATCH', 192))
    # num_workers is total workers
    num_workers = int(os.environ.get('SAICV_HP_WORKERS', 32))
    accumulation_steps = 1

    optimizer = ('AdamW', {'lr': 1e-4, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})

    epochs = int(os.environ.get('SAICV_HP_EPOCHS', 100))
    eval_epoch = [epochs]
    print_interval = int(os.environ.get('SAICV_HP_PRINT', 50))
    save_interval = 10

    save_model_metric = 'mean_iou'

    sync_bn = False
    use_amp = True
    use_compile = False
    compile_params = {'mode': 'default'}

    use_ema_model = False
    ema_model_decay = 0.9999
