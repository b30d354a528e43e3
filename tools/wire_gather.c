/* Side B of tools/wire_mixed_ab.py: what a node does today with a receive
 * buffer of mixed frames before the three single-kind fused calls -- one pass
 * over each frame's first four bytes (the bincode variant of PrimaryMessage)
 * and a gather of the frames into three contiguous batches, on one core.
 * Measurement only; compiled by the tool, not part of the engine. */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* out[k], out_offs[k] (count + 1 offsets), index[k] (the frame each item came
 * from), count[k] for k = Header, Vote, Certificate.  A frame shorter than
 * four bytes or of another variant goes nowhere. */
void wire_gather(const uint8_t* frames, const uint64_t* offs, size_t n, uint8_t* const out[3],
                 uint64_t* const out_offs[3], uint32_t* const index[3], size_t count[3]) {
  uint64_t end[3] = {0, 0, 0};
  for (int k = 0; k < 3; k++) {
    count[k] = 0;
    out_offs[k][0] = 0;
  }
  for (size_t i = 0; i < n; i++) {
    const size_t len = (size_t)(offs[i + 1] - offs[i]);
    if (len < 4) continue;
    const uint8_t* f = frames + offs[i];
    const uint32_t variant = (uint32_t)f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
    if (variant > 2) continue;
    memcpy(out[variant] + end[variant], f, len);
    end[variant] += len;
    index[variant][count[variant]] = (uint32_t)i;
    out_offs[variant][++count[variant]] = end[variant];
  }
}
