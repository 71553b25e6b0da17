from .encoder_decoder import EncoderDecoder  # noqa: F401
from .siam_encoder_decoder import SiamEncoderDecoder  # noqa: F401
