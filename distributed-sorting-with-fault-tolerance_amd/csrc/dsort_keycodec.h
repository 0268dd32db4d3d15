// dsort_keycodec.h -- the order-preserving key codec (dsort.h, "Key types and order"): one rule
// for the host (dsort_key_encode / dsort_key_decode) and for every kernel that reads the caller's
// keys or writes them back.
//
// A key's bits b, taken as an unsigned integer of the key's width W, become a word w whose SIGNED
// order is the wanted order of the keys:
//
//   I (int32, int64)       w = b
//   U (uint32, uint64)     w = b ^ sign_bit
//   F (float32, float64)   w = b ^ ((b >> (W-1)) & ~sign_bit), the shift arithmetic: a negative
//                          float flips every bit but the sign -- IEEE 754 totalOrder
//   descending             ~w of the ascending word
//
// Every step is an involution and none of the F rule's touches the sign bit it tests, so decoding
// is the same steps in reverse order and the round trip is bit-exact (NaN payloads, the sign of
// zero).  Two or three integer instructions per key.
//
// A codec is named by an id, cls + 3 * descending with cls 0 = I, 1 = U, 2 = F; id 0 is the
// identity.  The kernels take the id as a template parameter.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSORT_KC_HD __host__ __device__ __forceinline__
#else
#define DSORT_KC_HD inline
#endif

namespace dsort {
namespace kc {

constexpr int CLS_I = 0, CLS_U = 1, CLS_F = 2;
constexpr int NCODECS = 6;
constexpr int id_of(int cls, bool desc) { return cls + (desc ? 3 : 0); }

template <int KC>
struct Codec {
    static_assert(KC >= 0 && KC < NCODECS, "codec id");
    static constexpr int CLS = KC % 3;
    static constexpr bool DESC = KC >= 3;

    static DSORT_KC_HD uint32_t enc(uint32_t b) {
        uint32_t w = b;
        if (CLS == CLS_U) w = b ^ 0x80000000u;
        if (CLS == CLS_F) w = b ^ ((uint32_t)((int32_t)b >> 31) & 0x7FFFFFFFu);
        return DESC ? ~w : w;
    }
    static DSORT_KC_HD uint32_t dec(uint32_t w) {
        if (DESC) w = ~w;
        if (CLS == CLS_U) return w ^ 0x80000000u;
        if (CLS == CLS_F) return w ^ ((uint32_t)((int32_t)w >> 31) & 0x7FFFFFFFu);
        return w;
    }
    static DSORT_KC_HD uint64_t enc(uint64_t b) {
        uint64_t w = b;
        if (CLS == CLS_U) w = b ^ (1ull << 63);
        if (CLS == CLS_F) w = b ^ ((uint64_t)((int64_t)b >> 63) & ~(1ull << 63));
        return DESC ? ~w : w;
    }
    static DSORT_KC_HD uint64_t dec(uint64_t w) {
        if (DESC) w = ~w;
        if (CLS == CLS_U) return w ^ (1ull << 63);
        if (CLS == CLS_F) return w ^ ((uint64_t)((int64_t)w >> 63) & ~(1ull << 63));
        return w;
    }
};

// DSORT_KEY_* (dsort.h) -> class and width; false for an unknown type
inline bool type_info(int key_type, int *cls, int *bytes) {
    if (key_type < 0 || key_type > 5) return false;
    *cls = key_type % 3;
    *bytes = key_type < 3 ? 4 : 8;
    return true;
}

}  // namespace kc
}  // namespace dsort

// Runs the statement with KC_ a compile-time copy of the codec id `id`, 1..5 (the identity, 0, has
// the integer entry points' own kernels and is never dispatched here).
#define DSORT_KC_SWITCH(id, ...)                                \
    switch (id) {                                               \
        case 1: { constexpr int KC_ = 1; __VA_ARGS__; } break;  \
        case 2: { constexpr int KC_ = 2; __VA_ARGS__; } break;  \
        case 3: { constexpr int KC_ = 3; __VA_ARGS__; } break;  \
        case 4: { constexpr int KC_ = 4; __VA_ARGS__; } break;  \
        default: { constexpr int KC_ = 5; __VA_ARGS__; } break; \
    }
