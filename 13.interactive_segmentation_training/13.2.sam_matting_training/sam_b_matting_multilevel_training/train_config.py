"""Benchmark copy of reference 13.interactive_segmentation_training/13.2.sam_matting_training/sam_b_matting_multilevel_training/
train_config.py (:18-261): sam_b_matting at 1024, four decoder refinement iterations, single-prompt mode with point / box at 0.5
each, SAMMattingMultiLevelLoss (all eight weights 1, the mean over the four masks of every loss, mask_threshold 0.5), global batch 48 (6 per GPU on the
reference's 8), AdamW 1e-5 without weight decay, AMP, gradient-norm clipping 1.0, find_unused_parameters as the reference sets them;
the matting datasets + OpenCV transform block are replaced by a synthetic dataset and the SAM segmentation checkpoint is not loaded
(neither exists in the bench image).  SAICV_SAMMAT_{TRAIN,BATCH,WORKERS,EPOCHS,SIZE} shorten a run."""
import os
import sys

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.append(BASE_DIR)

from SimpleAICV.interactive_segmentation.models.segment_anything_matting import sam_matting
from SimpleAICV.interactive_segmentation import losses_matting
from SimpleAICV.interactive_segmentation.datasets.syntheticdataset import SyntheticSAMMattingDataset
from SimpleAICV.interactive_segmentation.common_matting import SAMMattingBatchCollater, load_state_dict


class config:
    network = 'sam_b_matting'
    input_image_size = int(os.environ.get('SAICV_SAMMAT_SIZE', 1024))
    mask_out_idxs = [0, 1, 2, 3]
    use_gradient_checkpoint = True
    frozen_image_encoder = False
    frozen_prompt_encoder = False
    frozen_mask_decoder = False
    mask_threshold = 0.5
    decoder_iters = 4

    model = sam_matting.__dict__[network](**{
        'image_size': input_image_size,
        'use_gradient_checkpoint': use_gradient_checkpoint,
        'frozen_image_encoder': frozen_image_encoder,
        'frozen_prompt_encoder': frozen_prompt_encoder,
        'frozen_mask_decoder': frozen_mask_decoder,
    })

    trained_model_path = ''
    load_state_dict(trained_model_path, model)

    use_single_prompt = True
    prompt_probs = {'prompt_point': 0.5, 'prompt_box': 0.5, 'prompt_mask': 0.}

    train_criterion = losses_matting.__dict__['SAMMattingMultiLevelLoss'](**{
        'global_pred_trimap_ce_loss_weight': 1,
        'global_pred_trimap_iou_loss_weight': 1,
        'local_pred_alpha_loss_weight': 1,
        'local_pred_laplacian_loss_weight': 1,
        'fusion_pred_alpha_loss_weight': 1,
        'fusion_pred_laplacian_loss_weight': 1,
        'composition_loss_weight': 1,
        'iou_predict_loss_weight': 1,
        'mask_threshold': mask_threshold,
    })

    train_dataset = SyntheticSAMMattingDataset(image_size=input_image_size, length=int(os.environ.get('SAICV_SAMMAT_TRAIN', 100000)),
                                               points_num=1, seed=0)
    train_collater = SAMMattingBatchCollater(resize=input_image_size)

    seed = 0
    batch_size = int(os.environ.get('SAICV_SAMMAT_BATCH', 48))
    num_workers = int(os.environ.get('SAICV_SAMMAT_WORKERS', 32))
    accumulation_steps = 1

    optimizer = ('AdamW', {'lr': 1e-5, 'global_weight_decay': False, 'weight_decay': 0,
                           'no_weight_decay_layer_name_list': []})
    scheduler = ('MultiStepLR', {'warm_up_epochs': 0, 'gamma': 0.1, 'milestones': [100]})

    epochs = int(os.environ.get('SAICV_SAMMAT_EPOCHS', 2))
    print_interval = 100
    save_interval = 1

    sync_bn = False
    use_amp = True
    use_compile = False
    compile_params = {'mode': 'default'}

    clip_max_norm = 1.

    find_unused_parameters = True
