/* tools/rollout_bench.py builds this into a shared library: the serial GAE loop on the host, compiled as the reference's
 * c_gae is.  The loop itself is tests/gae_serial.h's. */
#include "../tests/gae_serial.h"

void serial_gae(int n, float gamma, float lam, const float *d, const float *v, const float *r, float *adv) {
    gae_serial(n, gamma, lam, d, v, r, adv);
}
