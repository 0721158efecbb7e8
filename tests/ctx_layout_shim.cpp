// extern "C" face of rsparse_amd/csrc/wrmf_ctx_layout.h for tests/test_ctx_layout.py (compiled with g++ into pytest's tmp_path,
// like tests/cgp_quad_shim.cpp): the block edges, the sub-block storage and the pointer check of the multi-GPU context.
#include <cstdint>
#include <cstring>
#include <string>

#include "../rsparse_amd/csrc/wrmf_ctx_layout.h"

using namespace rsparse_hip;

extern "C" {

// p: n + 1 column pointers.  edges: ws + 1.  scal = {Bs, rows, ws, n_sub}.  sub_rows: ws x n_sub x {c0, c1}.  sub_start: ws x
// n_sub.  slab_start: n_sub.  storage: n (to_storage of every id).
void ctx_layout(const int32_t* p, int64_t n, int ws, int n_sub, int64_t* edges, int64_t* scal, int64_t* sub_rows, int64_t* sub_start,
                int64_t* slab_start, int64_t* storage) {
  const std::vector<int64_t> e = balanced_edges(p, n, ws);
  for (size_t r = 0; r < e.size(); r++) edges[r] = e[r];
  Lay lay;
  lay.init(n, e, n_sub);
  scal[0] = lay.Bs; scal[1] = lay.rows; scal[2] = lay.ws; scal[3] = lay.n_sub;
  for (int r = 0; r < lay.ws; r++)
    for (int j = 0; j < lay.n_sub; j++) {
      int64_t* sr = sub_rows + 2 * ((size_t)r * lay.n_sub + j);
      lay.sub_rows(r, j, sr[0], sr[1]);
      sub_start[(size_t)r * lay.n_sub + j] = lay.sub_start(r, j);
    }
  for (int j = 0; j < lay.n_sub; j++) slab_start[j] = lay.slab_start(j);
  for (int64_t g = 0; g < n; g++) storage[g] = lay.to_storage(g);
}

// 0 = both pointer arrays are accepted, 1 = refused with the text in msg
int ctx_check_ptrs(const int32_t* ui_p, int64_t n_item, const int32_t* iu_p, int64_t n_user, char* msg, int cap) {
  const std::string e = check_matrix_ptrs(ui_p, n_item, iu_p, n_user);
  if (msg && cap > 0) {
    std::strncpy(msg, e.c_str(), (size_t)cap - 1);
    msg[cap - 1] = 0;
  }
  return e.empty() ? 0 : 1;
}

}  // extern "C"
