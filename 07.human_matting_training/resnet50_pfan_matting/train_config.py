"""Benchmark copy of reference 07.human_matting_training/resnet50_pfan_matting/train_config.py (:19-146): network, 1024 x 1024
canvas, the seven matting losses at ratio 1.0, global batch 32, AdamW 1e-4, CosineLR with one warm-up epoch over 100 epochs, thresh
[0.2], squared_beta 0.3, checkpoints by miou_average, AMP, as the reference sets them; the human-matting dataset + OpenCV transform
block is replaced by a synthetic dataset of soft masks with derived trimaps and no pretrained backbone is loaded (neither exists in
the bench image)."""
import os
import sys

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(BASE_DIR)

from SimpleAICV.human_matting import models
from SimpleAICV.human_matting import losses
from SimpleAICV.human_matting.datasets.syntheticdataset import SyntheticHumanMattingDataset
from SimpleAICV.human_matting.common import HumanMattingCollater, load_state_dict


class config:
    # SAICV_MAT_* shorten a smoke run of the entry scripts
    input_image_size = [int(os.environ.get('SAICV_MAT_SIZE', 1024))] * 2
    network = 'resnet50_pfan_matting'

    backbone_pretrained_path = ''
    model = models.__dict__[network](**{'backbone_pretrained_path': backbone_pretrained_path})

    trained_model_path = ''
    load_state_dict(trained_model_path, model)

    loss_list = ['GlobalTrimapCELoss', 'GloabelTrimapIouLoss', 'LocalAlphaLoss', 'LocalLaplacianLoss', 'FusionAlphaLoss',
                 'FusionLaplacianLoss', 'CompositionLoss']
    loss_ratio = {loss_name: 1.0 for loss_name in loss_list}
    train_criterion = {loss_name: losses.__dict__[loss_name]() for loss_name in loss_list}
    test_criterion = losses.__dict__['GlobalTrimapCELoss']()

    train_dataset = SyntheticHumanMattingDataset(int(os.environ.get('SAICV_MAT_TRAIN', 30000)), input_image_size[0],
                                                 input_image_size[1], seed=0)
    # the complete validation set is the first entry of the list: the entry script checkpoints by its result
    val_dataset_name_list = [['P3M-500-NP', 'P3M-500-P']]
    val_dataset_list = []
    for per_sub_dataset_list in val_dataset_name_list:
        val_dataset_list.append(SyntheticHumanMattingDataset(int(os.environ.get('SAICV_MAT_TEST', 1000)), input_image_size[0],
                                                             input_image_size[1], seed=1 + len(val_dataset_list)))
    train_collater = HumanMattingCollater(resize=input_image_size[0])
    val_collater = HumanMattingCollater(resize=input_image_size[0])

    seed = 0
    # batch_size is total size
    batch_size = int(os.environ.get('SAICV_MAT_BATCH', 32))
    # num_workers is total workers
    num_workers = int(os.environ.get('SAICV_MAT_WORKERS', 32))
    accumulation_steps = 1

    optimizer = ('AdamW', {'lr': 1e-4, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})

    epochs = int(os.environ.get('SAICV_MAT_EPOCHS', 100))
    eval_epoch = [1] + [i for i in range(epochs) if i % 10 == 0]
    print_interval = int(os.environ.get('SAICV_MAT_PRINT', 100))
    save_interval = 10

    save_model_metric = 'miou_average'
    thresh = [0.2]
    squared_beta = 0.3

    sync_bn = False
    use_amp = True
    use_compile = False
    compile_params = {'mode': 'default'}
    use_step_graph = os.environ.get('SAICV_MAT_GRAPH', '0') == '1'

    use_ema_model = False
    ema_model_decay = 0.9999
