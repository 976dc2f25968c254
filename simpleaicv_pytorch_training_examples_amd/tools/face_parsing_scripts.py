"""Training / evaluation loops of the face-parsing family (reference tools/face_parsing_scripts.py, which is its
human_parsing_scripts.py under other names): the loops of tools/human_parsing_scripts.py under the reference's face names."""
from .human_parsing_scripts import first_dataset_metric, parsing_metrics  # noqa: F401
from .human_parsing_scripts import train_human_parsing as train_face_parsing  # noqa: F401
from .human_parsing_scripts import validate_human_parsing as validate_face_parsing  # noqa: F401
from .human_parsing_scripts import validate_human_parsing_for_all_dataset as validate_face_parsing_for_all_dataset  # noqa: F401
