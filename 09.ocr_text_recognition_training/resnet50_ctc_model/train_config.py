"""Benchmark copy of reference 09.ocr_text_recognition_training/resnet50_ctc_model/train_config.py (:20-170): CTCModel with
resnet50backbone and planes 512, 12 111 characters + blank (+ the garbage class: 12 113 outputs), CTCLoss without focal weight and
ratio 1.0, images of height 32, labels of at most 80 characters, global batch 512 with accumulation_steps 2, AdamW 1e-4, CosineLR
with one warm-up epoch over 50 epochs, evaluation at epochs 1, 10, 20, ..., checkpoints by lcs_precision, AMP, as the reference sets
them; the CNENTextRecognition datasets + OpenCV transform block are replaced by a synthetic dataset of 32 x 512 images with labels
of 1 to 24 characters of a generated table of the reference's size, and no trained model is loaded (none exists in the bench
image).  SAICV_OCR_* shorten a smoke run of the entry scripts; SAICV_OCR_VARIABLE_WIDTH=1 draws a width per sample."""
import os
import sys

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(BASE_DIR)

from SimpleAICV.text_recognition import losses
from SimpleAICV.text_recognition.char_sets.final_char_table import final_char_table
from SimpleAICV.text_recognition.common import CTCTextLabelConverter, KeepRatioResizeTextRecognitionCollater, load_state_dict
from SimpleAICV.text_recognition.datasets.syntheticdataset import SyntheticTextRecognitionDataset
from SimpleAICV.text_recognition.models import CTCModel


class config:
    network = 'CTCModel'
    resize_h = 32
    str_max_length = 80

    all_char_table = final_char_table
    converter = CTCTextLabelConverter(chars_set_list=final_char_table, str_max_length=str_max_length, garbage_char='㍿')
    # all char + '[CTCblank]' = 12111 + 1 = 12112; the model has one more output, the garbage class
    num_classes = converter.num_classes

    # rnn_route 'fused': ops.lstm instead of nn.LSTM -- the faster route at this shape, eagerly and in the captured step
    # (profiles/ocr_lstm.json); checkpoints are the same on either route
    model = CTCModel(backbone_type=os.environ.get('SAICV_OCR_BACKBONE', 'resnet50backbone'), planes=512, num_classes=num_classes + 1,
                     rnn_route='fused')

    trained_model_path = ''
    load_state_dict(trained_model_path, model)

    loss_list = {'CTCLoss': {'blank_index': num_classes - 1, 'use_focal_weight': False, 'gamma': 2.0}}
    loss_ratio = {'CTCLoss': 1.0}
    train_criterion = {}
    for loss_name, loss_param in loss_list.items():
        train_criterion[loss_name] = losses.__dict__[loss_name](**loss_param)
    test_criterion = losses.__dict__['CTCLoss'](**{'blank_index': num_classes - 1, 'use_focal_weight': False, 'gamma': 2.0})

    image_width = int(os.environ.get('SAICV_OCR_WIDTH', 512))
    variable_width = bool(int(os.environ.get('SAICV_OCR_VARIABLE_WIDTH', 0)))
    train_dataset = SyntheticTextRecognitionDataset(int(os.environ.get('SAICV_OCR_TRAIN', 512 * 200)), final_char_table, height=resize_h,
                                                    width=image_width, max_length=24, variable_width=variable_width, seed=0)
    val_dataset_name_list = [['synthetic_text']]
    val_dataset_list = []
    for i, per_sub_val_dataset_name in enumerate(val_dataset_name_list):
        val_dataset_list.append(SyntheticTextRecognitionDataset(int(os.environ.get('SAICV_OCR_TEST', 10000)), final_char_table,
                                                                height=resize_h, width=image_width, max_length=24,
                                                                variable_width=variable_width, seed=1 + i))
    train_collater = KeepRatioResizeTextRecognitionCollater(resize_h=resize_h)
    test_collater = KeepRatioResizeTextRecognitionCollater(resize_h=resize_h)

    seed = 0
    # batch_size is total size
    batch_size = int(os.environ.get('SAICV_OCR_BATCH', 512))
    # num_workers is total workers
    num_workers = int(os.environ.get('SAICV_OCR_WORKERS', 32))
    accumulation_steps = int(os.environ.get('SAICV_OCR_ACCUMULATION', 2))

    optimizer = ('AdamW', {'lr': 1e-4, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})

    epochs = int(os.environ.get('SAICV_OCR_EPOCHS', 50))
    print_interval = int(os.environ.get('SAICV_OCR_PRINT', 100))
    save_interval = 10
    eval_epoch = [1]
    for i in range(epochs):
        if i % 10 == 0:
            eval_epoch.append(i)

    save_model_metric = 'lcs_precision'

    sync_bn = False
    use_amp = True
    use_compile = False
    compile_params = {'mode': 'default'}

    use_ema_model = False
    ema_model_decay = 0.9999
