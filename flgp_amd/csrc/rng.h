// The counter RNG of flgp_amd/synth.py on the device, shared by pg.hip and nll.hip, so that numpy can regenerate every
// number a kernel consumes: stream st under seed has the base splitmix64(seed * 0x100000001B3 + st); its counter q gives
// the uniform ((splitmix64(base + q) >> 11) + 0.5) 2^-53; normal p of a stream is Box-Muller on the uniforms 2p, 2p + 1,
// sqrt(-2 log u_2p) cos(2 pi u_2p+1).  Nothing depends on the launch geometry.
#pragma once
#include <hip/hip_runtime.h>

namespace flgp {

__host__ __device__ inline unsigned long long rng_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline unsigned long long rng_stream_base(unsigned long long seed, unsigned long long stream) {
  return rng_mix(seed * 0x100000001B3ull + stream);
}
__device__ __forceinline__ double rng_unif(unsigned long long base, unsigned long long q) {
  return ((double)(rng_mix(base + q) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double rng_box_muller(double u1, double u2) {
  return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}

}  // namespace flgp
