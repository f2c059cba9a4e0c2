// att32_tile_row.h -- text of att32_tile.h, included at the top of the tile loop: takes the geometry that gstage prefetched.
// This lane's row of the tile is (point t0 + row / KN = pp[row / KN], neighbour row % KN = nbr), row = c32.
int pp[PPT];
#pragma unroll
for (int i = 0; i < PPT; ++i) pp[i] = n_pp[i];
const int nbr = n_nl;
const float rx = n_c[0] - n_n[0], ry = n_c[1] - n_n[1], rz = n_c[2] - n_n[2];
const float dis = __builtin_amdgcn_sqrtf(rx * rx + ry * ry + rz * rz);
const float enc[10] = {dis, rx, ry, rz, n_c[0], n_c[1], n_c[2], n_n[0], n_n[1], n_n[2]};  // relative_pos_encoding's ten inputs of LocSE
