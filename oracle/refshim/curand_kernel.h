/* curand_kernel.h -- TEST INFRASTRUCTURE (oracle/refshim).  The reference's kernel file includes this header and uses nothing of
 * it: its generator is its own sampler.h. */
