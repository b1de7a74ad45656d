// The per-sample arithmetic of PCM decode and encode (include/viai_hip.h, "WAV in, WAV out"), written ONCE: the kernels of wav_io.hip and the
// host mirrors viai_pcm_*_host call these same functions, so the same bits on the host and on the device are a property of the source.
// A sample travels as its RAW value: the little-endian integer its 1, 2, 3, 4 or 8 bytes spell.  fp32 only apart from the two fp64 casts;
// every product is a single rounded fp32 operation (contraction is off below this line, no fast-math flag in the Makefile), the scalings by
// powers of two are exact, rintf is round-half-even on both sides and hipcc's fp32 divide is the correctly rounded one.
#pragma once
#pragma clang fp contract(off)

#define PCM_HD __host__ __device__ inline

// bytes per sample; 0 for an unknown format
PCM_HD int pcm_bytes(int fmt) {
    return fmt == VIAI_PCM_U8 ? 1 : fmt == VIAI_PCM_S16 ? 2 : fmt == VIAI_PCM_S24 ? 3 : (fmt == VIAI_PCM_S32 || fmt == VIAI_PCM_F32) ? 4
         : fmt == VIAI_PCM_F64 ? 8 : 0;
}

// 1. decode: raw -> fp32.  Bits of raw above the sample's width are ignored.
PCM_HD float pcm_decode(int fmt, unsigned long long raw) {
    switch (fmt) {
    case VIAI_PCM_U8:
        return (float)((int)(raw & 0xffu) - 128) / 128.f;
    case VIAI_PCM_S16:
        return (float)(short)(raw & 0xffffu) / 32768.f;
    case VIAI_PCM_S24: {
        const int v = (int)((unsigned)(raw & 0xffffffu) << 8) >> 8;       // sign extension of bit 23
        return (float)v / 8388608.f;
    }
    case VIAI_PCM_S32:
        return (float)(int)(unsigned)raw * 4.656612873077392578125e-10f;  // nearest even, then 2^-31 (exact)
    case VIAI_PCM_F32:
        return __builtin_bit_cast(float, (unsigned)raw);
    default:
        return (float)__builtin_bit_cast(double, raw);
    }
}
PCM_HD bool pcm_finite(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7fffffffu) < 0x7f800000u; }

// the mono downmix: the caller adds the channels in order in fp32, ((x0 + x1) + ...) + x_{C-1}; this is the one division behind it
PCM_HD float pcm_mono(float sum, int channels) { return sum / (float)channels; }

// 2. encode, plain: fp32 -> raw.  Integer formats round to nearest even and clamp IN FLOAT before the conversion, so x >= 1 is the maximum and
// never wraps; a non-finite x is 0 (128 for U8).
PCM_HD int pcm_round_clamp(float x, float scale, float hi, int imax, int imin) {
    if (!pcm_finite(x)) return 0;
    const float y = __builtin_rintf(x * scale);
    return y >= hi ? imax : (y <= -scale ? imin : (int)y);
}
PCM_HD unsigned long long pcm_encode(int fmt, float x) {
    switch (fmt) {
    case VIAI_PCM_U8:
        return (unsigned long long)(unsigned)(pcm_round_clamp(x, 128.f, 127.f, 127, -128) + 128);
    case VIAI_PCM_S16:
        return (unsigned long long)((unsigned)pcm_round_clamp(x, 32768.f, 32767.f, 32767, -32768) & 0xffffu);
    case VIAI_PCM_S24:
        return (unsigned long long)((unsigned)pcm_round_clamp(x, 8388608.f, 8388607.f, 8388607, -8388608) & 0xffffffu);
    case VIAI_PCM_S32:
        return (unsigned long long)(unsigned)pcm_round_clamp(x, 2147483648.f, 2147483648.f, 2147483647, -2147483647 - 1);
    case VIAI_PCM_F32:
        return (unsigned long long)__builtin_bit_cast(unsigned, x);
    default:
        return __builtin_bit_cast(unsigned long long, (double)x);
    }
}

// 3. encode, normalised (S16 only; the reference's save_wav): peak is max |x| over the finite samples
PCM_HD float pcm_norm_scale(float peak) { return (double)peak <= 0.01 ? 3276700.0f : 32767.0f / peak; }
PCM_HD unsigned long long pcm_encode_norm(float x, float scale) {
    if (!pcm_finite(x)) return 0ull;
    const float y = x * scale;                                            // |y| < 32768 for every |x| <= peak
    return (unsigned long long)((unsigned)(int)y & 0xffffu);              // the conversion truncates
}
