"""`from paddle.regularizer import L2Decay` (gvt.py:7, levit.py:9, ghostnet.py:12): imported by name, never used in eval mode."""


class L2Decay:
    def __init__(self, coeff=0.0):
        self.coeff = coeff
