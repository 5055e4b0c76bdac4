"""Case module: the AV-MNIST shaped tables."""
from oracle import np_oracle as O


SS, VS = (3, 6, 12, 24, 48), (3, 6, 12)


def tables():
    return (O.synth_table(192, 71, snr=1.0, C=10, s_sizes=SS, v_sizes=VS),
            O.synth_table(96, 72, snr=1.0, C=10, s_sizes=SS, v_sizes=VS))
