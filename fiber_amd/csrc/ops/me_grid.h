// The behaviour grid of the MAP-Elites archive, passed to me_assign by
// value.  Dimension d has bins[d] bins over [lo[d], lo[d] + bins[d] /
// inv[d]); inv is rounded to fp32 on the host from double precision.
#pragma once

struct MeGrid {
  float lo[4];
  float inv[4];
  int bins[4];
};
