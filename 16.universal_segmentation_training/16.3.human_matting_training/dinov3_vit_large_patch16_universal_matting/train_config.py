"""Benchmark copy of reference 16.universal_segmentation_training/16.3.human_matting_training/
dinov3_vit_large_patch16_universal_matting/train_config.py (:20-115): network, 1024-pixel canvas, 100 queries, 2 classes (background
included), UniversalMattingLoss with every cost and weight 1 and no-object weight 0.1, global batch 32 in 4 accumulation steps,
('Muon', lr 4e-4, weight decay 1e-3), CosineLR with one warm-up epoch over 50 epochs, AMP, as the reference sets them; the human
matting datasets + OpenCV resize are replaced by a synthetic matte dataset at its final size and no pretrained backbone is loaded
(neither exists in the bench image).  SAICV_UNIMAT_* shorten a smoke run of the entry script."""
import os
import sys

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.append(BASE_DIR)

from SimpleAICV.universal_segmentation import models
from SimpleAICV.universal_segmentation import matting_losses
from SimpleAICV.universal_segmentation.datasets.syntheticmattingdataset import SyntheticUniversalMattingDataset
from SimpleAICV.universal_segmentation.human_matting_common import (HumanMattingTrainCollater, Normalize, RandomHorizontalFlip,
                                                                    load_state_dict)


class _Compose:

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, sample):
        for t in self.transforms:
            sample = t(sample)
        return sample


class config:
    network = os.environ.get('SAICV_UNIMAT_MODEL', 'dinov3_vit_large_patch16_universal_matting')
    query_num = int(os.environ.get('SAICV_UNIMAT_QUERIES', 100))
    # num_classes has background class
    num_classes = 2
    input_image_size = [int(os.environ.get('SAICV_UNIMAT_SIZE', 1024))] * 2

    backbone_pretrained_path = ''
    model = models.dinov3_universal_matting.__dict__[network](**{
        'backbone_pretrained_path': backbone_pretrained_path,
        'image_size': input_image_size[0],
        'query_num': query_num,
        'num_classes': num_classes,
    })

    trained_model_path = ''
    load_state_dict(trained_model_path, model)

    train_criterion = matting_losses.__dict__['UniversalMattingLoss'](**{
        'global_trimap_ce_cost': 1.0,
        'global_trimap_iou_cost': 1.0,
        'local_alpha_cost': 1.0,
        'fusion_alpha_cost': 1.0,
        'class_cost': 1.0,
        'num_classes': num_classes,
        'global_trimap_ce_loss_weight': 1.0,
        'global_trimap_iou_loss_weight': 1.0,
        'local_alpha_loss_weight': 1.0,
        'local_laplacian_loss_weight': 1.0,
        'fusion_alpha_loss_weight': 1.0,
        'fusion_laplacian_loss_weight': 1.0,
        'class_loss_weight': 1.0,
        'no_object_class_weight': 0.1,
    })

    train_dataset = SyntheticUniversalMattingDataset(int(os.environ.get('SAICV_UNIMAT_TRAIN', 20000)), input_image_size[0], seed=0,
                                                     transform=_Compose([RandomHorizontalFlip(prob=0.5), Normalize()]))
    train_collater = HumanMattingTrainCollater(resize=input_image_size[0])

    seed = 0
    # batch_size is total size
    batch_size = int(os.environ.get('SAICV_UNIMAT_BATCH', 32))
    # num_workers is total workers
    num_workers = int(os.environ.get('SAICV_UNIMAT_WORKERS', 32))
    accumulation_steps = int(os.environ.get('SAICV_UNIMAT_ACCUM', 4))

    optimizer = ('Muon', {'lr': 4e-4, 'weight_decay': 1e-3, 'exclude_muon_layer_name_list': []})
    scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})

    epochs = int(os.environ.get('SAICV_UNIMAT_EPOCHS', 50))
    print_interval = int(os.environ.get('SAICV_UNIMAT_PRINT', 100))
    save_interval = 10

    sync_bn = False
    use_amp = True
    use_compile = False
    compile_params = {'mode': 'default'}

    use_ema_model = False
    ema_model_decay = 0.9999
