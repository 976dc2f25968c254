"""A character table of the reference's size, generated: 10 digits, 52 letters and a run of CJK Unified Ideographs from U+4E00,
12 111 characters in all, so that CTCTextLabelConverter(final_char_table).num_classes == 12112 and the model has 12 113 outputs
(the reference's resnet50_ctc_model config).  The reference's own table is a literal list of the same length; a training run on
real text puts that list here."""
import string

NUM_CHARS = 12111

num_and_alpha_char_table = list(string.digits + string.ascii_uppercase + string.ascii_lowercase)
final_char_table = num_and_alpha_char_table + [chr(0x4E00 + i) for i in range(NUM_CHARS - len(num_and_alpha_char_table))]
