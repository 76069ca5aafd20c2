// host_contour.hpp -- the host half of the contour eigensolver (host_contour.cpp, plain C++) besides the C ABI's
// emme_contour_eigs: the argument rules, the count, the candidates and the kept roots of a region search, and its round
// plan ContourRounds.  The plan is the search: search_contours (contour.hip), the one driver behind
// emme_find_roots_in_contour and emme_find_roots_in_contours_sets, only carries out on the device what the plan asks
// for -- which nodes exist, where they sit, what they weigh and when L doubles is decided here and nowhere else.
#pragma once
#include <vector>

#include "../../include/emme_hip.h"

namespace emme {

// Winding number of det M along a closed contour from arg det M at its nodes, in contour order (args[j] at t_j,
// N >= 2, any branch of the angle): W = sum_j wrap(arg_{j+1} - arg_j) / 2 pi, the last difference closing the
// curve.  *resolved = every |wrapped step| <= max_step and |W - round W| <= 0.05.  Returns round(W).
int contour_winding(const double* args, int N, double max_step, bool* resolved, double* W_raw);

// The argument rules of a region search on one contour: nullptr if ct passes, else what is wrong with it (the text
// after the entry point's name in emme_last_error).
const char* contour_arg_error(const emme_contour_t* ct);

// One polished candidate of a region search and what its chain reported.
struct ContourRoot {
    double re, im;
    int it, inf;
    int chain;  // which of the ng candidates it was
};
// The roots a region search keeps of its ng polished candidates r (chains its / inf, iterates `path` with
// step_limit + 1 entries per chain): converged, inside the ellipse, no duplicate (10 tol |omega|) of an earlier
// one; sorted by Im omega descending.
std::vector<ContourRoot> contour_keep_roots(const emme_contour_t& ct, double tol, int step_limit, int ng, const double* r,
                                            const int* its, const int* inf, const double* path);
// The candidates mu (k of them, normalised by rho = max(a, b) around the centre) that may be eigenvalues inside the
// ellipse: finite, normalised radius below 1.5.  Appended to guesses as (re, im); kept (nullable): their positions in
// mu, appended likewise.
void contour_candidates(const emme_contour_t& ct, int k, const double* mu, std::vector<double>& guesses,
                        std::vector<int>* kept = nullptr);

// The round plan of a region search over many (parameter set, contour) items that advance in lock step (DESIGN.md
// §13.9).  No device: the caller fills, factors and solves what the plan asks for and hands the log-dets and ranks
// back.  Nodes are numbered over the whole call in the order they are created; an item's own nodes do not depend on
// the other items of the call: the search on one contour is the call with one item.  set null (that search): every
// item's set is 0 and r_set is not to be read.
struct ContourRounds {
    struct Item {
        int set = 0;
        emme_contour_t ct{};
        int N = 0;              // nodes so far (0 before the first round)
        int L = 0;              // probe columns solved at every node of the item
        int W = -1;             // the count, once resolved
        int k = 0;              // numerical rank of the last moments
        int status = 0;         // EMME_OK, or the error that took the item out
        bool adding = true;     // the item adds nodes in the next node round
        bool doubling = true;   // the item takes part in the next moment pass
        bool dropped = false;
        std::vector<int> nodes;   // the nodes it owns, in creation order
        std::vector<int> node_m;  // node j of the item sits at t = 2 pi node_m[j] / max_points
    };
    std::vector<Item> items;
    std::vector<int> node_item;  // the owner of every node

    // the fill batch of the current node round: node r_first + q belongs to item r_item[q], set r_set[q], and sits at
    // (r_omega[2q], r_omega[2q + 1])
    int r_first = 0;
    std::vector<int> r_item, r_set;
    std::vector<double> r_omega;

    ContourRounds(int nitems, const int* set, const emme_contour_t* contours);
    int nodes() const { return (int)node_item.size(); }
    // 1. which items add which nodes: the start nodes of every item at first, later the midpoints of the items whose
    // count is unresolved below their max_points.  False: no item adds nodes any more (nothing planned).
    bool plan_nodes();
    // an item leaves the call (a failed node fill, a failed Beyn step): winding -1, no roots, no further work
    void drop(int item, int status);
    // 2. the arguments of det M at every node so far (logdet: (log|det|, arg det) per node): each item that is still
    // adding decides its count on its own nodes
    void take_logdets(const double* logdet);
    // 3. the moment pass: the items still doubling L (`which`), their node lists (item which[g] sums idx[off[g]] ..
    // idx[off[g + 1] - 1], in the item's creation order, nodes with info != 0 left out) and the weights (w, z) of
    // every node of those items, indexed by node (4 doubles each; wz has 4 nodes() entries)
    bool plan_moments(const int* info, std::vector<int>& which, std::vector<int>& off, std::vector<int>& idx,
                      std::vector<double>& wz) const;
    // the rank of an item's moments: true if the item doubles L, then columns [*l0, *l0 + *nl) are to be solved at its
    // nodes (and L is already the new count)
    bool take_rank(int item, int k, int* l0, int* nl);
};

}  // namespace emme
