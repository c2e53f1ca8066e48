#pragma once
#include <stdint.h>

#include "common.h"

namespace twr {
// ---------------------------------------------------------------- a new grid_map layer for a live batch
// twr_batch_grid_map_sync / twr_batch_grid_map_update_device: the batch's copy of a `Grid` elevation layer (the buffer
// DevStruct::grid_ptr names; its address never changes) is overwritten from a layer with any start index, and the new map
// centre goes into the header of every structure of the batch that reads this map.
//
// A moved grid_map is a circular buffer: cell (i, j) of the map lies at buffer index ((i + start_x) mod size_x,
// (j + start_y) mod size_y) (grid_map's published getBufferIndexFromIndex), column-major.  The batch keeps start index
// (0,0), which is what gridmap_sample (terrain.h) reads, so column j of the batch's copy is column (j + start_y) mod size_y
// of the source, rotated by start_x: two contiguous runs,
//   dst[0, size_x - start_x)      = src[start_x, size_x)
//   dst[size_x - start_x, size_x) = src[0, start_x)
// One wave copies one column, run by run: lane l takes elements l, l + 64, ... of a run, so both the reads and the writes of a
// wave instruction are consecutive dwords, and the only wrap arithmetic is one compare per column.  A run's first element
// sits at any dword (size_x and start_x are arbitrary), so the accesses stay 4 bytes wide; the `e < len` bound is the tail
// lane's, for a run shorter than a wave as well.  Cells are moved as 32-bit words: NaN cells keep their payload.
// 7-160 KB per call: the launch, not the copy, is what it costs.
TWR_DEV void grid_map_copy_run(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int len, int lane) {
  for (int e = lane; e < len; e += 64) dst[e] = src[e];
}
// Column j of the batch's copy, by the wave that calls it (lane = 0 .. 63).  0 <= start_x < size_x, 0 <= start_y < size_y.
TWR_DEV void grid_map_unroll_column(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int size_x, int size_y,
                                    int start_x, int start_y, int j, int lane) {
  int js = j + start_y;
  if (js >= size_y) js -= size_y;
  const uint32_t* s = src + (int64_t)js * size_x;
  uint32_t* d = dst + (int64_t)j * size_x;
  const int head = size_x - start_x;   // >= 1
  grid_map_copy_run(s + start_x, d, head, lane);
  grid_map_copy_run(s, d + head, start_x, lane);
}
// The map centre of header k of the map's list: hdr_off[k] is the byte offset of DevStruct::grid_px in the batch's arena
// (grid_py follows it), from the list twr_batch_create built.  Plain 8-byte stores.
TWR_DEV void grid_map_put_centre(char* __restrict__ arena, const uint64_t* __restrict__ hdr_off, int k, double pos_x, double pos_y) {
  double* c = reinterpret_cast<double*>(arena + hdr_off[k]);
  c[0] = pos_x;
  c[1] = pos_y;
}
}  // namespace twr
