// The live taps of FBI_Net's masked convolutions (archs/comp.py:281, 294), shared by the forward kernels (fbinet.hip) and the training
// kernels (fbinet_train.hip).  Tap t sits at (r[t], c[t]) of a K x K kernel at dilation DIL: offset ((r - K / 2) DIL, (c - K / 2) DIL).
// Every set is point-symmetric: tap t mirrors to tap N - 1 - t.
#pragma once

// tap set 0: the 9 knight-and-centre taps of the masked 5x5 (archs/comp.py:281), set 1: centre and corners of the 3x3 at dilation 3 (:294)
template <int SET> struct FbiTaps;
template <> struct FbiTaps<0> {
    static constexpr int N = 9, HALO = 2, K = 5, DIL = 1;
    static constexpr int r[9] = {0, 0, 1, 1, 2, 3, 3, 4, 4};        // (row, column) in the 5x5 kernel
    static constexpr int c[9] = {1, 3, 0, 4, 2, 0, 4, 1, 3};
};
template <> struct FbiTaps<1> {
    static constexpr int N = 5, HALO = 3, K = 3, DIL = 3;
    static constexpr int r[9] = {0, 0, 1, 2, 2, 0, 0, 0, 0};        // (row, column) in the 3x3 kernel
    static constexpr int c[9] = {0, 2, 1, 0, 2, 0, 0, 0, 0};
};
// set 2: a 1x1 convolution seen as a one-tap set (the residual modules' GEMMs in the weight-gradient kernel)
template <> struct FbiTaps<2> {
    static constexpr int N = 1, HALO = 0, K = 1, DIL = 1;
    static constexpr int r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    static constexpr int c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};
